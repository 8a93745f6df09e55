// The similarity metrics of SFMA on the device (memory/utils/metrics.py:66-268 of the reference):
// SR.D = inv(I - gamma T) and DR.D = D0 - D0[:, J] (I + delta D0[:, J])^-1 delta D0 for stacks of
// four-action worlds given by their compact successor tables.  Everything is float64 with one
// rounding per operation and every sum in ascending index order (no MFMA: a fused accumulate rounds
// once where the contract rounds twice), so the matrices equal the NumPy restatement of
// tests/metric_common.py bit for bit.
//
// cobel_metric_sr   k_metric_init writes L = I - gamma T straight from the table (T[s][c] = count /
//                   4, exact; no dense T exists), then the blocked in-place Gauss-Jordan of
//                   cobel_gj.h: per panel of 32 pivots the tiles, the lines, the diagonal block,
//                   ordered by the stream; the world is the grid's z axis.
//                   1 + 3 ceil(S / 32) launches (S <= 32: two).
// cobel_metric_dr   four launches on a caller-owned workspace:
//   k_dr_alpha      one workgroup per world: the rows delta[i] = (I - gamma T_new)[J_i] -
//                   (I - gamma T_default)[J_i] on their at most nine columns, A = I_k + delta
//                   D0[:, J] and alpha = A^-1 by in-place Gauss-Jordan with partial pivoting in LDS
//                   (largest magnitude in the column, lowest row on ties; the row swaps are undone
//                   as column swaps in reverse order at the end)
//   k_dr_x          X = delta D0            [k][S]
//   k_dr_y          Y = D0[:, J] alpha      [S][k]
//   k_dr_update     D = D0 - Y X over 64 x 64 tiles: D0 read once, D written once, Y and X staged
//                   through LDS 32 terms at a time (k = 0: D = D0)
#include "cobel_gj.h"

namespace {

using namespace cobel_gj;

constexpr int kNnz = 9;          // columns of a row of delta: the state, 4 new and 4 default successors
constexpr int kChunk = 32;       // terms of Y X staged at a time

struct sr_args {
  double* D;             // [W][S][S]
  const int32_t* next;   // [W][S][4]
  double gamma;
  int32_t S, k0, kb, nbr;
};

__global__ __launch_bounds__(kThreads) void k_metric_init(const sr_args P) {
  const int S = P.S;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (size_t)S * S) return;
  const size_t w = blockIdx.z;
  const int r = (int)(e / (size_t)S), c = (int)(e - (size_t)r * S);
  const int32_t* const nx = P.next + (w * (size_t)S + (size_t)r) * 4;
  int cnt = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) cnt += nx[a] == c ? 1 : 0;
  const double t = (double)cnt * 0.25;
  P.D[w * (size_t)S * S + e] = (r == c ? 1.0 : 0.0) - P.gamma * t;
}

__global__ __launch_bounds__(kThreads) void k_metric_tiles(const sr_args P) {
  extern __shared__ __attribute__((aligned(16))) double gj_lds[];
  gj_tiles(P.D + (size_t)blockIdx.z * P.S * P.S, P.S, P.k0, P.kb, gj_lds);
}
__global__ __launch_bounds__(kThreads) void k_metric_lines(const sr_args P) {
  extern __shared__ __attribute__((aligned(16))) double gj_lds[];
  gj_lines(P.D + (size_t)blockIdx.z * P.S * P.S, P.S, P.k0, P.kb, P.nbr, gj_lds);
}
__global__ __launch_bounds__(kThreads) void k_metric_diag(const sr_args P) {
  extern __shared__ __attribute__((aligned(16))) double gj_lds[];
  gj_diag(P.D + (size_t)blockIdx.z * P.S * P.S, P.S, P.k0, P.kb, gj_lds);
}

// ---- DR -------------------------------------------------------------------------------------------
// Workspace: rank [W] and J [W][kmax] (int32, together rounded up to 16 bytes), then per world
// dcol int32 [kmax][9] (rounded up to 8 bytes), dval [kmax][9], alpha [k][k], X [k][S], Y [S][k]
// (doubles; the last three packed by the world's own rank k), the world's part rounded up to 16.
__host__ __device__ inline size_t dr_head_bytes(int W, int kmax) {
  return ((size_t)4 * W * (1 + (size_t)kmax) + 15) / 16 * 16;
}
__host__ __device__ inline size_t dr_dcol_bytes(int kmax) {
  return ((size_t)4 * kNnz * kmax + 7) / 8 * 8;
}
__host__ __device__ inline size_t dr_world_bytes(int S, int kmax) {
  const size_t k = (size_t)kmax;
  return (dr_dcol_bytes(kmax) + 8 * (kNnz * k + k * k + 2 * k * (size_t)S) + 15) / 16 * 16;
}

struct dr_args {
  const double* D0;        // [S][S]
  const int32_t* next;     // [W][S][4]
  const int32_t* next_def; // [S][4]
  double* D;               // [W][S][S]
  char* work;
  double gamma;
  int32_t S, W, kmax;
};

struct dr_world {
  int k;
  const int32_t* J;
  int32_t* dcol;
  double *dval, *alpha, *X, *Y;
};
__device__ __forceinline__ dr_world dr_carve(const dr_args& P, int w) {
  dr_world v;
  const int32_t* const rank = reinterpret_cast<const int32_t*>(P.work);
  v.k = rank[w];
  v.J = rank + P.W + (size_t)w * P.kmax;
  char* const base = P.work + dr_head_bytes(P.W, P.kmax) + (size_t)w * dr_world_bytes(P.S, P.kmax);
  v.dcol = reinterpret_cast<int32_t*>(base);
  v.dval = reinterpret_cast<double*>(base + dr_dcol_bytes(P.kmax));
  v.alpha = v.dval + (size_t)kNnz * P.kmax;
  v.X = v.alpha + (size_t)v.k * v.k;
  v.Y = v.X + (size_t)v.k * P.S;
  return v;
}

// LDS of k_dr_alpha for ranks up to k: A [k][k | 1], col [k], row [k], the reduction's values [256],
// dval [k][9]; then int32: the reduction's rows [256], piv [k], dcol [k][9], J [k]
constexpr size_t alpha_lds_bytes(int k) {
  return 8 * ((size_t)k * (k | 1) + 2 * (size_t)k + kThreads + (size_t)kNnz * k) +
         4 * ((size_t)kThreads + k + (size_t)kNnz * k + k);
}
static_assert(alpha_lds_bytes(COBEL_METRIC_MAX_RANK) <= 160 * 1024,
              "COBEL_METRIC_MAX_RANK: the k x k block and its bookkeeping must fit one workgroup's LDS");

__global__ __launch_bounds__(kThreads) void k_dr_alpha(const dr_args P) {
  extern __shared__ __attribute__((aligned(16))) double a_lds[];
  const int w = (int)blockIdx.z, t = (int)threadIdx.x, S = P.S;
  const dr_world V = dr_carve(P, w);
  const int k = V.k;
  if (k == 0) return;
  const int ld = k | 1;
  double* const A = a_lds;
  double* const col = A + (size_t)k * ld;
  double* const row = col + k;
  double* const redv = row + k;
  double* const dval = redv + kThreads;
  int32_t* const redi = reinterpret_cast<int32_t*>(dval + kNnz * k);
  int32_t* const piv = redi + kThreads;
  int32_t* const dcol = piv + k;
  int32_t* const Js = dcol + kNnz * k;
  if (t < k) Js[t] = V.J[t];
  // delta: the columns of row J[t] in ascending order, then the values
  if (t < k) {
    const int j = V.J[t];
    const int32_t* const nn = P.next + ((size_t)w * S + (size_t)j) * 4;
    const int32_t* const nd = P.next_def + (size_t)j * 4;
    int cand[kNnz], cols[kNnz], n = 0;
    cand[0] = j;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      cand[1 + a] = nn[a];
      cand[5 + a] = nd[a];
    }
    for (int q = 0; q < kNnz; ++q) {
      const int x = cand[q];
      if (x < 0 || x >= S) continue;
      int pos = 0;
      while (pos < n && cols[pos] < x) ++pos;
      if (pos < n && cols[pos] == x) continue;
      for (int m = n; m > pos; --m) cols[m] = cols[m - 1];
      cols[pos] = x;
      ++n;
    }
    for (int s = 0; s < kNnz; ++s) {
      int c = -1;
      double v = 0.0;
      if (s < n) {
        c = cols[s];
        int cn = 0, cd = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          cn += nn[a] == c ? 1 : 0;
          cd += nd[a] == c ? 1 : 0;
        }
        const double e = c == j ? 1.0 : 0.0;
        v = (e - P.gamma * ((double)cn * 0.25)) - (e - P.gamma * ((double)cd * 0.25));
      }
      dcol[t * kNnz + s] = c;
      dval[t * kNnz + s] = v;
      V.dcol[t * kNnz + s] = c;
      V.dval[t * kNnz + s] = v;
    }
  }
  __syncthreads();
  // A = I_k + delta D0[:, J]
  for (int e = t; e < k * k; e += kThreads) {
    const int i = e / k, jj = e - i * k;
    const size_t cj = (size_t)Js[jj];
    double acc = 0.0;
    for (int s = 0; s < kNnz; ++s) {
      const int c = dcol[i * kNnz + s];
      const double v = dval[i * kNnz + s];
      if (c >= 0 && v != 0.0) acc = acc + v * P.D0[(size_t)c * S + cj];
    }
    A[i * ld + jj] = (i == jj ? 1.0 : 0.0) + acc;
  }
  // alpha = A^-1
  for (int kk = 0; kk < k; ++kk) {
    __syncthreads();
    redv[t] = (t < k && t >= kk) ? fabs(A[t * ld + kk]) : -1.0;
    redi[t] = t;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if (t < s) {
        const double vo = redv[t + s], vm = redv[t];
        const int io = redi[t + s], im = redi[t];
        if (vo > vm || (vo == vm && io < im)) {
          redv[t] = vo;
          redi[t] = io;
        }
      }
      __syncthreads();
    }
    int p = redi[0];
    if (p < kk || p >= k) p = kk;    // (a column of NaNs: no row wins a comparison)
    if (p != kk && t < k) {
      const double x = A[kk * ld + t];
      A[kk * ld + t] = A[p * ld + t];
      A[p * ld + t] = x;
    }
    if (t == 0) piv[kk] = p;
    __syncthreads();
    const double inv = 1.0 / A[kk * ld + kk];
    if (t < k) col[t] = A[t * ld + kk];
    else if (t >= 128 && t - 128 < k) {
      const int j = t - 128;
      row[j] = (j == kk ? 1.0 : A[kk * ld + j]) * inv;
    }
    __syncthreads();
    for (int e = t; e < k * k; e += kThreads) {
      const int i = e / k, j = e - i * k;
      const double r = row[j];
      if (i == kk) A[i * ld + j] = r;
      else A[i * ld + j] = (j == kk ? 0.0 : A[i * ld + j]) - col[i] * r;
    }
  }
  __syncthreads();
  for (int kk = k - 1; kk >= 0; --kk) {
    const int p = piv[kk];
    if (p != kk && t < k) {
      const double x = A[t * ld + kk];
      A[t * ld + kk] = A[t * ld + p];
      A[t * ld + p] = x;
    }
    __syncthreads();
  }
  for (int e = t; e < k * k; e += kThreads) {
    const int i = e / k, j = e - i * k;
    V.alpha[e] = A[i * ld + j];
  }
}

// grid (ceil(S / 256), kmax, W): X[i][c] = sum over the columns cc of delta[i], ascending, of
// delta[i][cc] D0[cc][c]
__global__ __launch_bounds__(kThreads) void k_dr_x(const dr_args P) {
  const int w = (int)blockIdx.z, i = (int)blockIdx.y, S = P.S;
  const dr_world V = dr_carve(P, w);
  const int c = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= V.k || c >= S) return;
  double acc = 0.0;
  for (int s = 0; s < kNnz; ++s) {
    const int cc = V.dcol[i * kNnz + s];
    const double v = V.dval[i * kNnz + s];
    if (cc >= 0 && v != 0.0) acc = acc + v * P.D0[(size_t)cc * S + c];
  }
  V.X[(size_t)i * S + c] = acc;
}

// grid (ceil(S kmax / 256), 1, W): Y[r][j] = sum over i ascending of D0[r][J[i]] alpha[i][j]
__global__ __launch_bounds__(kThreads) void k_dr_y(const dr_args P) {
  const int w = (int)blockIdx.z, S = P.S;
  const dr_world V = dr_carve(P, w);
  const int k = V.k;
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= (size_t)S * k) return;
  const int r = (int)(e / (size_t)k), j = (int)(e - (size_t)r * k);
  const double* const d0 = P.D0 + (size_t)r * S;
  double acc = 0.0;
  for (int i = 0; i < k; ++i) acc = acc + d0[V.J[i]] * V.alpha[(size_t)i * k + j];
  V.Y[e] = acc;
}

constexpr size_t kUpdateDoubles = (size_t)kChunk * kTileLd + (size_t)kChunk * kTile;
// grid (ceil(S / 64), ceil(S / 64), W): D = D0 - Y X
__global__ __launch_bounds__(kThreads) void k_dr_update(const dr_args P) {
  __shared__ double Ys[kChunk * kTileLd];   // Ys[ii][r] = Y[R0 + r][i0 + ii]
  __shared__ double Xs[kChunk * kTile];     // Xs[ii][c] = X[i0 + ii][C0 + c]
  const int w = (int)blockIdx.z, t = (int)threadIdx.x, S = P.S;
  const dr_world V = dr_carve(P, w);
  const int k = V.k;
  const int R0 = (int)blockIdx.y * kTile, C0 = (int)blockIdx.x * kTile;
  const int tr = (t / 16) * 4, tc = (t % 16) * 4;
  double b[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) b[i][j] = 0.0;
  for (int i0 = 0; i0 < k; i0 += kChunk) {
    const int kc = k - i0 < kChunk ? k - i0 : kChunk;
    __syncthreads();
    for (int e = t; e < kTile * kc; e += kThreads) {
      const int r = e / kc, ii = e - r * kc;
      Ys[ii * kTileLd + r] = R0 + r < S ? V.Y[(size_t)(R0 + r) * k + i0 + ii] : 0.0;
    }
    for (int e = t; e < kc * kTile; e += kThreads) {
      const int ii = e / kTile, c = e - ii * kTile;
      Xs[ii * kTile + c] = C0 + c < S ? V.X[(size_t)(i0 + ii) * S + C0 + c] : 0.0;
    }
    __syncthreads();
    for (int ii = 0; ii < kc; ++ii) {
      double a[4], x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Ys[ii * kTileLd + tr + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = Xs[ii * kTile + tc + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[i][j] = b[i][j] + a[i] * x[j];
    }
  }
  double* const D = P.D + (size_t)w * S * S;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = R0 + tr + i, c = C0 + tc + j;
      if (r < S && c < S) {
        const double d0 = P.D0[(size_t)r * S + c];
        D[(size_t)r * S + c] = k == 0 ? d0 : d0 - b[i][j];
      }
    }
}

int check_common(const char* who, int32_t n_worlds, int32_t n_states, double gamma) {
  COBEL_REQUIRE(n_worlds >= 1, COBEL_E_ARG, "%s: n_worlds = %d (at least one world)", who, n_worlds);
  COBEL_REQUIRE(gamma >= 0.0 && gamma < 1.0, COBEL_E_ARG,
                "%s: gamma = %g outside [0, 1): the elimination without pivoting rests on the "
                "diagonal dominance of I - gamma T", who, gamma);
  COBEL_REQUIRE(n_states >= 1 && n_states <= COBEL_METRIC_MAX_STATES, COBEL_E_UNSUPPORTED,
                "%s: %d states; the device metrics serve 1 .. %d states", who, n_states,
                COBEL_METRIC_MAX_STATES);
  COBEL_REQUIRE(n_worlds <= COBEL_METRIC_MAX_WORLDS, COBEL_E_UNSUPPORTED,
                "%s: %d worlds; one call takes up to %d worlds", who, n_worlds,
                COBEL_METRIC_MAX_WORLDS);
  return COBEL_OK;
}

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

}  // namespace

extern "C" {

int cobel_metric_plan(int32_t n_states, int32_t rank, int64_t out[4]) {
  COBEL_REQUIRE(out != nullptr, COBEL_E_ARG, "cobel_metric_plan: out is NULL");
  out[0] = out[1] = out[2] = out[3] = 0;
  COBEL_REQUIRE(n_states >= 1 && n_states <= COBEL_METRIC_MAX_STATES, COBEL_E_UNSUPPORTED,
                "cobel_metric_plan: %d states; the device metrics serve 1 .. %d states", n_states,
                COBEL_METRIC_MAX_STATES);
  COBEL_REQUIRE(rank >= 0 && rank <= COBEL_METRIC_MAX_RANK, COBEL_E_UNSUPPORTED,
                "cobel_metric_plan: rank %d; the LDS of one workgroup holds ranks 0 .. %d", rank,
                COBEL_METRIC_MAX_RANK);
  size_t lds = 8 * (n_states <= kB ? kDiagDoubles
                                   : (kTileDoubles > kLineDoubles ? kTileDoubles : kLineDoubles));
  if (rank > 0) {
    if (alpha_lds_bytes(rank) > lds) lds = alpha_lds_bytes(rank);
    if (8 * kUpdateDoubles > lds) lds = 8 * kUpdateDoubles;
  }
  out[0] = n_states <= kB ? 0 : 1;
  out[1] = (int64_t)lds;
  out[2] = kThreads;
  out[3] = (int64_t)dr_world_bytes(n_states, rank);
  return COBEL_OK;
}

int cobel_metric_sr(const int32_t* next, int32_t n_worlds, int32_t n_states, double gamma,
                    double* D, void* stream) {
  COBEL_REQUIRE(next != nullptr && D != nullptr, COBEL_E_ARG, "cobel_metric_sr: %s is NULL",
                next == nullptr ? "next" : "D");
  COBEL_REQUIRE(!misaligned(next, 4) && !misaligned(D, 8), COBEL_E_ARG,
                "cobel_metric_sr: misaligned pointer");
  if (const int rc = check_common("cobel_metric_sr", n_worlds, n_states, gamma)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = n_states;
  const unsigned nz = (unsigned)n_worlds;
  const unsigned nt = (unsigned)((S + kTile - 1) / kTile);
  const int nbr = (S + kThreads - 1) / kThreads;
  const unsigned init_blocks = (unsigned)(((size_t)S * S + kThreads - 1) / kThreads);
  sr_args P;
  P.D = D;
  P.next = next;
  P.gamma = gamma;
  P.S = S;
  P.k0 = 0;
  P.kb = 0;
  P.nbr = nbr;
  COBEL_HIP_TRY(cobel_launch(k_metric_init, dim3(init_blocks, 1, nz), dim3(kThreads), 0, st, P));
  for (int k0 = 0; k0 < S; k0 += kB) {
    P.k0 = k0;
    P.kb = S - k0 < kB ? S - k0 : kB;
    if (S > P.kb) {   // (else the diagonal block is the whole matrix)
      COBEL_HIP_TRY(cobel_launch(k_metric_tiles, dim3(nt, nt, nz), dim3(kThreads), 8 * kTileDoubles,
                                 st, P));
      COBEL_HIP_TRY(cobel_launch(k_metric_lines, dim3(2u * (unsigned)nbr, 1, nz), dim3(kThreads),
                                 8 * kLineDoubles, st, P));
    }
    COBEL_HIP_TRY(cobel_launch(k_metric_diag, dim3(1, 1, nz), dim3(kThreads), 8 * kDiagDoubles, st,
                               P));
  }
  return COBEL_OK;
}

int cobel_metric_dr(const double* D0, const int32_t* next, const int32_t* next_default,
                    const int32_t* J, const int32_t* rank, int32_t max_rank, int32_t n_worlds,
                    int32_t n_states, double gamma, double* D, void* work, int64_t work_bytes,
                    void* stream) {
  const char* const who = "cobel_metric_dr";
  COBEL_REQUIRE(D0 && next && next_default && rank && D && work, COBEL_E_ARG,
                "%s: %s is NULL", who,
                !D0 ? "D0" : !next ? "next" : !next_default ? "next_default" : !rank ? "rank"
                : !D ? "D" : "work");
  COBEL_REQUIRE(!misaligned(D0, 8) && !misaligned(D, 8) && !misaligned(next, 4) &&
                    !misaligned(next_default, 4) && !misaligned(work, 16),
                COBEL_E_ARG, "%s: misaligned pointer", who);
  COBEL_REQUIRE(D != D0, COBEL_E_ARG, "%s: D must not be D0", who);
  if (const int rc = check_common(who, n_worlds, n_states, gamma)) return rc;
  COBEL_REQUIRE(max_rank >= 0, COBEL_E_ARG, "%s: max_rank = %d", who, max_rank);
  COBEL_REQUIRE(max_rank <= COBEL_METRIC_MAX_RANK, COBEL_E_UNSUPPORTED,
                "%s: rank %d; the LDS of one workgroup holds ranks up to %d", who, max_rank,
                COBEL_METRIC_MAX_RANK);
  COBEL_REQUIRE(max_rank == 0 || J != nullptr, COBEL_E_ARG, "%s: J is NULL", who);
  for (int w = 0; w < n_worlds; ++w) {
    const int k = rank[w];
    COBEL_REQUIRE(k <= COBEL_METRIC_MAX_RANK, COBEL_E_UNSUPPORTED,
                  "%s: world %d has rank %d; the LDS of one workgroup holds ranks up to %d", who, w,
                  k, COBEL_METRIC_MAX_RANK);
    COBEL_REQUIRE(k >= 0 && k <= max_rank, COBEL_E_ARG, "%s: world %d has rank %d, max_rank is %d",
                  who, w, k, max_rank);
    const int32_t* const Jw = J + (size_t)w * max_rank;
    for (int i = 0; i < k; ++i) {
      COBEL_REQUIRE(Jw[i] >= 0 && Jw[i] < n_states, COBEL_E_ARG,
                    "%s: world %d: J[%d] = %d is no state of a world of %d", who, w, i, Jw[i],
                    n_states);
      COBEL_REQUIRE(i == 0 || Jw[i - 1] < Jw[i], COBEL_E_ARG,
                    "%s: world %d: J is not sorted (J[%d] = %d after %d)", who, w, i, Jw[i],
                    Jw[i - 1]);
    }
  }
  const size_t need = dr_head_bytes(n_worlds, max_rank) +
                      (size_t)n_worlds * dr_world_bytes(n_states, max_rank);
  COBEL_REQUIRE(work_bytes >= 0 && (size_t)work_bytes >= need, COBEL_E_ARG,
                "%s: a workspace of %lld bytes; %d worlds of %d states at rank %d take %zu bytes",
                who, (long long)work_bytes, n_worlds, n_states, max_rank, need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = n_states;
  const unsigned nz = (unsigned)n_worlds;
  char* const wk = static_cast<char*>(work);
  COBEL_HIP_TRY(hipMemcpyAsync(wk, rank, (size_t)4 * n_worlds, hipMemcpyHostToDevice, st));
  if (max_rank > 0)
    COBEL_HIP_TRY(hipMemcpyAsync(wk + (size_t)4 * n_worlds, J, (size_t)4 * n_worlds * max_rank,
                                 hipMemcpyHostToDevice, st));
  dr_args P;
  P.D0 = D0;
  P.next = next;
  P.next_def = next_default;
  P.D = D;
  P.work = wk;
  P.gamma = gamma;
  P.S = S;
  P.W = n_worlds;
  P.kmax = max_rank;
  if (max_rank > 0) {
    COBEL_HIP_TRY(cobel_launch(k_dr_alpha, dim3(1, 1, nz), dim3(kThreads),
                               alpha_lds_bytes(max_rank), st, P));
    COBEL_HIP_TRY(cobel_launch(k_dr_x, dim3((unsigned)((S + kThreads - 1) / kThreads),
                                            (unsigned)max_rank, nz),
                               dim3(kThreads), 0, st, P));
    const unsigned yb = (unsigned)(((size_t)S * max_rank + kThreads - 1) / kThreads);
    COBEL_HIP_TRY(cobel_launch(k_dr_y, dim3(yb, 1, nz), dim3(kThreads), 0, st, P));
  }
  const unsigned nt = (unsigned)((S + kTile - 1) / kTile);
  COBEL_HIP_TRY(cobel_launch(k_dr_update, dim3(nt, nt, nz), dim3(kThreads), 0, st, P));
  return COBEL_OK;
}

}  // extern "C"
