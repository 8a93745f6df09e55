// PMAMemory.compute_need(None) beyond the LDS, cobel_pma_stationary_wide: the solve of
// k_pma_stationary (pma_need.hip) on a workspace in device memory, for 1 .. 1 024 states.  Every
// element goes through the operations of that kernel in the same order, one rounding each
// (-ffp-contract=off), so the result equals tests/pma_need_common.py: stationary_ref bit for bit,
// and the LDS kernel's wherever both run:
//   fill     A[r][c] = ((r == c ? 1 : 0) - T[c][r]) + 1 / S,  A[r][S] = 1 / S
//   pivot k  the largest |A[r][k]|, r >= k, the lowest r among equals, a NaN never; an exactly zero
//            pivot makes the instance degenerate
//   update   A[r][c] = A[r][c] - f[r] * A[k][c], f[r] = A[r][k] / pivot, r > k, k < c <= S, k ascending
//   back     k = S - 1 .. 0: x[k] = b[k] / A[k][k]; b[r] = b[r] - A[r][k] * x[k], r < k
//   norm     a = |x|; the squares summed by the power-of-two tree; need = a / sqrt(sum)
//
// Workspace per instance (caller-owned): the augmented matrix A [S][S + 1] (column S the right-hand
// side), the pivot rows int32 [S] and one int32 mark (1: degenerate), rounded up to 16 bytes.  The
// elimination is a right-looking LU in place, blocked over panels K = [k0, k0 + kb) of kPanel
// pivots; per panel three launches, ordered by the stream (no kernel waits for another workgroup):
//   k_need_panel  one workgroup per instance: columns K, rows k0 .. S - 1 in LDS, the kb steps with
//                 pivoting; the multipliers stay in the dead lower part (a row swap moves them with
//                 the row), the pivot rows go to the workspace; a zero pivot sets the mark
//   k_need_urows  one lane per column c right of the panel (column S included): the panel's swaps in
//                 that column, then rows K of U: A[k][c] - f_j[k] * A[j][c], j = k0 .. k - 1 ascending
//   k_need_tiles  one workgroup per 64 x 64 tile of the rest, so one instance spreads over the chip:
//                 A[r][c] - f_j[r] * A[j][c], j ascending over K, from the panel's multipliers and
//                 the rows of U staged in LDS
// An element right of the panel meets the swaps first and the updates afterwards instead of
// interleaved: a swap moves a row's values and its multipliers together, so the element that ends
// in a place sees the operations it would have seen on its way there.  Columns left of the panel
// are dead (nothing reads a multiplier of an earlier panel again) and are not swapped.
//   k_need_fill   32 x 32 tiles of T transposed through LDS; clears the mark
//   k_need_back   one workgroup per instance: b and x in LDS, U by 64 x 64 diagonal blocks — the block
//                 in LDS for its own 64 steps, then one lane per row above it, k descending
// Later launches skip an instance whose mark is set; k_need_back then writes status 1 and the
// uniform vector.  Instances whose select entry is >= 0 leave every kernel at once.  The entry point
// takes the instances in groups of as many as the workspace holds; a group's launches follow the
// previous group's in the stream, and no element's operations depend on the grouping.
#include "cobel_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPanel = 16;              // pivots per panel
constexpr int kPanelLd = kPanel + 1;    // odd: lanes on consecutive rows of a column hit different banks
constexpr int kTile = 64;
constexpr int kTileLd = kTile + 1;
constexpr int kFill = 32;
constexpr int kBack = 64;               // columns per block of the back substitution
constexpr int kBackLd = kBack + 1;
constexpr int kMaxS = COBEL_PMA_WIDE_MAX_STATES;
static_assert(kPanel <= 64 && kBack <= kThreads, "one wave swaps a panel row; one lane per block row");

__host__ __device__ inline int wide_ld(int S) { return S + 1; }
__host__ __device__ inline int wide_pow2(int S) {
  int p = 1;
  while (p < S) p *= 2;
  return p;
}
__host__ __device__ inline size_t wide_work_bytes(int S) {
  const size_t b = 8 * (size_t)S * wide_ld(S) + 4 * ((size_t)S + 1);
  return (b + 15) & ~(size_t)15;
}
size_t panel_lds(int S) { return 8 * (size_t)S * kPanelLd; }
constexpr size_t kUrowsLds = 8 * (size_t)kPanel * kPanel + 4 * kPanel;
constexpr size_t kTilesLds = 8 * ((size_t)kPanel * kTileLd + (size_t)kPanel * kTile);
constexpr size_t kFillLds = 8 * (size_t)kFill * (kFill + 1);
size_t back_lds(int S) { return 8 * ((size_t)kBack * kBackLd + 2 * (size_t)S + wide_pow2(S)) + 8; }

struct wide_args {
  const double* T;          // [N][S][S]
  const int32_t* select;    // [N] or NULL
  double* need;             // [N][S]
  int32_t* status;          // [N]
  char* work;               // [group][wide_work_bytes(S)]
  int32_t S, k0, kb;
  uint32_t inst0;           // the group's first instance; blockIdx.z counts from it
};

struct wide_slot {
  double* A;
  int32_t* piv;
  int32_t* mark;
};
__device__ __forceinline__ wide_slot slot_of(const wide_args& P) {
  wide_slot s;
  s.A = reinterpret_cast<double*>(P.work + (size_t)blockIdx.z * wide_work_bytes(P.S));
  s.piv = reinterpret_cast<int32_t*>(s.A + (size_t)P.S * wide_ld(P.S));
  s.mark = s.piv + P.S;
  return s;
}
__device__ __forceinline__ bool skipped(const wide_args& P) {
  return P.select && P.select[P.inst0 + blockIdx.z] >= 0;
}

__global__ __launch_bounds__(kThreads) void k_need_fill(const wide_args P) {
  if (skipped(P)) return;
  __shared__ double tile[kFill][kFill + 1];
  const wide_slot w = slot_of(P);
  const int S = P.S, ld = wide_ld(S), t = (int)threadIdx.x;
  const int tx = t % kFill, ty = t / kFill;
  const int C0 = (int)blockIdx.x * kFill, R0 = (int)blockIdx.y * kFill;
  const double* const T = P.T + (size_t)(P.inst0 + blockIdx.z) * S * S;
  const double inv_s = 1.0 / (double)S;
  // T is read along its rows, which are the columns of A
  for (int i = ty; i < kFill; i += kThreads / kFill) {
    const int c = C0 + i, r = R0 + tx;
    tile[i][tx] = (c < S && r < S) ? T[(size_t)c * S + r] : 0.0;
  }
  __syncthreads();
  for (int i = ty; i < kFill; i += kThreads / kFill) {
    const int r = R0 + i, c = C0 + tx;
    if (r < S && c < S) w.A[(size_t)r * ld + c] = ((r == c ? 1.0 : 0.0) - tile[tx][i]) + inv_s;
  }
  if (blockIdx.x == 0) {
    if (t < kFill && R0 + t < S) w.A[(size_t)(R0 + t) * ld + S] = inv_s;
    if (blockIdx.y == 0 && t == 0) *w.mark = 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_need_panel(const wide_args P) {
  if (skipped(P)) return;
  const wide_slot w = slot_of(P);
  if (*w.mark != 0) return;
  extern __shared__ __attribute__((aligned(16))) double wide_lds[];
  double* const Ap = wide_lds;                 // [h][kPanelLd] Ap[r][j] = A[k0 + r][k0 + j]
  const int S = P.S, ld = wide_ld(S), k0 = P.k0, kb = P.kb, h = S - k0;
  const int t = (int)threadIdx.x, lane = t & 63;
  for (int e = t; e < h * kb; e += kThreads) {
    const int r = e / kb, j = e - r * kb;
    Ap[r * kPanelLd + j] = w.A[(size_t)(k0 + r) * ld + k0 + j];
  }
  __syncthreads();
  for (int kk = 0; kk < kb; ++kk) {
    // every wave reduces the column for itself: the same values give the same row
    double bv = -1.0;
    int bi = kk;
    for (int r = kk + lane; r < h; r += 64) {
      const double v = fabs(Ap[r * kPanelLd + kk]);
      if (v > bv) {
        bv = v;
        bi = r;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = __shfl_xor(bv, m);
      const int oi = __shfl_xor(bi, m);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    const int p = __builtin_amdgcn_readfirstlane(bi);
    const double pv = Ap[p * kPanelLd + kk];
    if (pv == 0.0) {     // (the same for every lane of the workgroup)
      if (t == 0) *w.mark = 1;
      return;
    }
    __syncthreads();     // (every wave has read the column before the swap moves it)
    if (t < kb && p != kk) {
      const double a = Ap[kk * kPanelLd + t];
      Ap[kk * kPanelLd + t] = Ap[p * kPanelLd + t];
      Ap[p * kPanelLd + t] = a;
    }
    if (t == 64) w.piv[k0 + kk] = k0 + p;
    __syncthreads();
    // a lane per row: its multiplier into the dead column, then its elements of the panel
    for (int r = kk + 1 + t; r < h; r += kThreads) {
      double* const row = Ap + r * kPanelLd;
      const double f = row[kk] / pv;
      row[kk] = f;
      for (int c = kk + 1; c < kb; ++c) row[c] = row[c] - f * Ap[kk * kPanelLd + c];
    }
    __syncthreads();
  }
  for (int e = t; e < h * kb; e += kThreads) {
    const int r = e / kb, j = e - r * kb;
    w.A[(size_t)(k0 + r) * ld + k0 + j] = Ap[r * kPanelLd + j];
  }
}

__global__ __launch_bounds__(kThreads) void k_need_urows(const wide_args P) {
  if (skipped(P)) return;
  const wide_slot w = slot_of(P);
  if (*w.mark != 0) return;
  __shared__ double Ls[kPanel][kPanel];        // Ls[i][j] = f_j[k0 + i], j < i
  __shared__ int32_t pivs[kPanel];
  const int S = P.S, ld = wide_ld(S), k0 = P.k0, kb = P.kb, k1 = k0 + kb;
  const int t = (int)threadIdx.x;
  if (t < kPanel * kPanel) {
    const int i = t / kPanel, j = t % kPanel;
    Ls[i][j] = (i < kb && j < i) ? w.A[(size_t)(k0 + i) * ld + k0 + j] : 0.0;
  }
  if (t < kPanel) pivs[t] = t < kb ? w.piv[k0 + t] : 0;
  __syncthreads();
  const int c = k1 + (int)blockIdx.x * kThreads + t;
  if (c > S) return;
  double* const col = w.A + c;
  for (int kk = 0; kk < kb; ++kk) {
    const int p = pivs[kk];
    if (p != k0 + kk) {
      const double a = col[(size_t)(k0 + kk) * ld];
      col[(size_t)(k0 + kk) * ld] = col[(size_t)p * ld];
      col[(size_t)p * ld] = a;
    }
  }
  double u[kPanel];
#pragma unroll
  for (int i = 0; i < kPanel; ++i) u[i] = i < kb ? col[(size_t)(k0 + i) * ld] : 0.0;
#pragma unroll
  for (int j = 0; j < kPanel; ++j)
#pragma unroll
    for (int i = j + 1; i < kPanel; ++i) u[i] = u[i] - Ls[i][j] * u[j];
#pragma unroll
  for (int i = 1; i < kPanel; ++i)
    if (i < kb) col[(size_t)(k0 + i) * ld] = u[i];
}

__global__ __launch_bounds__(kThreads) void k_need_tiles(const wide_args P) {
  if (skipped(P)) return;
  const wide_slot w = slot_of(P);
  if (*w.mark != 0) return;
  __shared__ double Fs[kPanel][kTileLd];       // Fs[j][r] = f_j[R0 + r]
  __shared__ double Us[kPanel][kTile];         // Us[j][c] = A[k0 + j][C0 + c]
  const int S = P.S, ld = wide_ld(S), k0 = P.k0, kb = P.kb, k1 = k0 + kb;
  const int t = (int)threadIdx.x;
  const int R0 = k1 + (int)blockIdx.y * kTile, C0 = k1 + (int)blockIdx.x * kTile;
  for (int e = t; e < kTile * kb; e += kThreads) {
    const int r = e / kb, j = e - r * kb;
    Fs[j][r] = R0 + r < S ? w.A[(size_t)(R0 + r) * ld + k0 + j] : 0.0;
  }
  for (int e = t; e < kb * kTile; e += kThreads) {
    const int j = e / kTile, c = e - j * kTile;
    Us[j][c] = C0 + c <= S ? w.A[(size_t)(k0 + j) * ld + C0 + c] : 0.0;
  }
  __syncthreads();
  // lane (t / 16, t % 16) holds 4 x 4 elements: rows tr + 16 i (a half wave reads 16 rows of a
  // column of Fs), columns tc .. tc + 3
  const int tr = t / 16, tc = (t % 16) * 4;
  double m[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = R0 + tr + 16 * i, c = C0 + tc + j;
      m[i][j] = (r < S && c <= S) ? w.A[(size_t)r * ld + c] : 0.0;
    }
  for (int kk = 0; kk < kb; ++kk) {
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = Fs[kk][tr + 16 * i];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = Us[kk][tc + j];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) m[i][j] = m[i][j] - a[i] * b[j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = R0 + tr + 16 * i, c = C0 + tc + j;
      if (r < S && c <= S) w.A[(size_t)r * ld + c] = m[i][j];
    }
}

__global__ __launch_bounds__(kThreads) void k_need_back(const wide_args P) {
  if (skipped(P)) return;
  const wide_slot w = slot_of(P);
  extern __shared__ __attribute__((aligned(16))) double wide_lds[];
  const int S = P.S, ld = wide_ld(S), P2 = wide_pow2(S);
  const int t = (int)threadIdx.x;
  const size_t inst = (size_t)P.inst0 + blockIdx.z;
  double* const Dg = wide_lds;                 // [kBack][kBackLd] the diagonal block of U
  double* const B = Dg + kBack * kBackLd;      // [S] the right-hand side
  double* const X = B + S;                     // [S] the solution
  double* const F = X + S;                     // [P2] the tree of squares
  int* const flag = reinterpret_cast<int*>(F + P2);
  bool bad = *w.mark != 0;                     // (the same for every lane of the workgroup)
  if (!bad) {
    for (int r = t; r < S; r += kThreads) B[r] = w.A[(size_t)r * ld + S];
    if (t == 0) *flag = 0;
    for (int kA = ((S - 1) / kBack) * kBack; kA >= 0; kA -= kBack) {
      const int bw = S - kA < kBack ? S - kA : kBack;
      __syncthreads();
      for (int e = t; e < bw * bw; e += kThreads) {
        const int i = e / bw, j = e - i * bw;
        Dg[i * kBackLd + j] = w.A[(size_t)(kA + i) * ld + kA + j];
      }
      __syncthreads();
      for (int kk = bw - 1; kk >= 0; --kk) {
        const double xk = B[kA + kk] / Dg[kk * kBackLd + kk];
        if (t < kk) B[kA + t] = B[kA + t] - Dg[t * kBackLd + kk] * xk;
        else if (t == kk) X[kA + kk] = xk;
        __syncthreads();
      }
      for (int r = t; r < kA; r += kThreads) {
        const double* const row = w.A + (size_t)r * ld + kA;
        double b = B[r];
        for (int kk = bw - 1; kk >= 0; --kk) b = b - row[kk] * X[kA + kk];
        B[r] = b;
      }
    }
    __syncthreads();
    for (int j = t; j < P2; j += kThreads) {
      const double a = j < S ? fabs(X[j]) : 0.0;
      F[j] = a * a;
    }
    __syncthreads();
    for (int hh = P2 / 2; hh >= 1; hh >>= 1) {
      for (int j = t; j < hh; j += kThreads) F[j] = F[j] + F[j + hh];
      __syncthreads();
    }
    const double norm = sqrt(F[0]);
    for (int j = t; j < S; j += kThreads) {
      const double v = fabs(X[j]) / norm;
      B[j] = v;
      if (!__builtin_isfinite(v)) *flag = 1;
    }
    __syncthreads();
    bad = *flag != 0;
  }
  const double uniform = 1.0 / sqrt((double)S);
  for (int j = t; j < S; j += kThreads) P.need[inst * S + j] = bad ? uniform : B[j];
  if (t == 0) P.status[inst] = bad ? 1 : 0;
}

size_t wide_largest_lds(int S) {
  size_t b = panel_lds(S);
  if (back_lds(S) > b) b = back_lds(S);
  if (kTilesLds > b) b = kTilesLds;
  if (kFillLds > b) b = kFillLds;
  if (kUrowsLds > b) b = kUrowsLds;
  return b;
}

}  // namespace

extern "C" int cobel_pma_plan_need_wide(int32_t n_states, int64_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_pma_plan_need_wide: NULL out");
  out[0] = out[1] = out[2] = out[3] = 0;
  COBEL_REQUIRE(n_states >= 1 && n_states <= kMaxS, COBEL_E_UNSUPPORTED,
                "cobel_pma_plan_need_wide: %d states (the workspace form of the stationary "
                "distribution is served for 1 to %d states)",
                n_states, kMaxS);
  out[0] = (int64_t)wide_work_bytes(n_states);
  out[1] = (int64_t)wide_largest_lds(n_states);
  out[2] = kThreads;
  out[3] = kPanel;
  return COBEL_OK;
}

extern "C" int cobel_pma_stationary_wide(const cobel_pma_mem_t* mem, const int32_t* select,
                                         double* need, int32_t* status, void* work,
                                         int64_t work_bytes, void* stream) {
  COBEL_REQUIRE(mem, COBEL_E_ARG, "cobel_pma_stationary_wide: NULL mem");
  COBEL_REQUIRE(mem->n_states >= 1 && mem->n_states <= kMaxS, COBEL_E_UNSUPPORTED,
                "cobel_pma_stationary_wide: %d states (the workspace form of the stationary "
                "distribution is served for 1 to %d states)",
                mem->n_states, kMaxS);
  COBEL_REQUIRE(mem->n >= 1, COBEL_E_RANGE, "cobel_pma_stationary_wide: n = %d", mem->n);
  COBEL_REQUIRE(mem->T && need && status && work, COBEL_E_ARG,
                "cobel_pma_stationary_wide: T, need, status and work are required");
  COBEL_REQUIRE((((uintptr_t)mem->T | (uintptr_t)need | (uintptr_t)work) & 7u) == 0 &&
                    (((uintptr_t)select | (uintptr_t)status) & 3u) == 0,
                COBEL_E_ARG, "cobel_pma_stationary_wide: misaligned argument");
  const int S = mem->n_states;
  const size_t per = wide_work_bytes(S);
  COBEL_REQUIRE(work_bytes >= (int64_t)per, COBEL_E_ARG,
                "cobel_pma_stationary_wide: a workspace of %lld bytes; one instance of %d states "
                "needs %lld bytes",
                (long long)work_bytes, S, (long long)per);
  const hipStream_t st = (hipStream_t)stream;
  uint32_t group = (uint32_t)((size_t)work_bytes / per < 65535u ? (size_t)work_bytes / per : 65535u);
  if (group > (uint32_t)mem->n) group = (uint32_t)mem->n;
  const unsigned nf = (unsigned)((S + kFill - 1) / kFill);
  wide_args P;
  P.T = mem->T;
  P.select = select;
  P.need = need;
  P.status = status;
  P.work = static_cast<char*>(work);
  P.S = S;
  for (uint32_t inst0 = 0; inst0 < (uint32_t)mem->n; inst0 += group) {
    const unsigned nz = (uint32_t)mem->n - inst0 < group ? (uint32_t)mem->n - inst0 : group;
    P.inst0 = inst0;
    P.k0 = P.kb = 0;
    COBEL_HIP_TRY(cobel_launch(k_need_fill, dim3(nf, nf, nz), dim3(kThreads), 0, st, P));
    for (int k0 = 0; k0 < S; k0 += kPanel) {
      P.k0 = k0;
      P.kb = S - k0 < kPanel ? S - k0 : kPanel;
      const int k1 = k0 + P.kb;
      COBEL_HIP_TRY(cobel_launch(k_need_panel, dim3(1, 1, nz), dim3(kThreads), panel_lds(S - k0),
                                 st, P));
      // columns k1 .. S: the right-hand side is always among them
      COBEL_HIP_TRY(cobel_launch(k_need_urows, dim3((unsigned)((S - k1) / kThreads + 1), 1, nz),
                                 dim3(kThreads), 0, st, P));
      if (k1 < S)
        COBEL_HIP_TRY(cobel_launch(k_need_tiles,
                                   dim3((unsigned)((S - k1) / kTile + 1),
                                        (unsigned)((S - k1 + kTile - 1) / kTile), nz),
                                   dim3(kThreads), 0, st, P));
    }
    COBEL_HIP_TRY(cobel_launch(k_need_back, dim3(1, 1, nz), dim3(kThreads), back_lds(S), st, P));
  }
  return COBEL_OK;
}
