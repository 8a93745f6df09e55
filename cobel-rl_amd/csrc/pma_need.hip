// PMAMemory.compute_need(None) (memory/pma.py:403-408) as a device call, cobel_pma_stationary: per
// instance |v| for the unit-2-norm left eigenvector v of T for the eigenvalue 1.  T is row-stochastic
// (memory/pma.py:139, :163-166), so v is the stationary distribution pi of T divided by its 2-norm,
// and pi solves
//     (I - T + (1/S) 1 1^T)^T x = (1/S) 1
// (pi (I - T) = 0 and pi 1 = 1; the matrix is regular whenever the eigenvalue 1 is simple, i.e. for
// every unichain T, transient states included).  No eigen-solver: one dense elimination.
//
// k_pma_stationary: one workgroup of 256 lanes per instance.  The augmented matrix — S rows of
// S + 1 doubles, column S the right-hand side — stays in LDS for the whole solve, with the
// multipliers, the pivots and the solution beside it.  The row stride is the next ODD count of
// doubles past S: the pivot search and the multipliers read a column with consecutive lanes on
// consecutive rows, and an odd stride of doubles puts the 32 lanes of a half wave on 32 different
// pairs of banks.  Every operation is float64 with one rounding (-ffp-contract=off; double division
// and sqrt are correctly rounded) in a fixed order, so tests/pma_need_common.py restates the kernel
// in NumPy bit for bit:
//   fill     A[r][c] = ((r == c ? 1 : 0) - T[c][r]) + 1 / S,  A[r][S] = 1 / S
//   pivot k  the largest |A[r][k]|, r >= k, the lowest r among equals (every wave reduces the column
//            for itself: the same values give the same row, and no barrier is needed to tell it);
//            an exactly zero pivot ends the solve as degenerate
//   swap     rows k and p in the columns past k (column k is read once more, for the multipliers,
//            and is dead afterwards: the pivot goes to D[k])
//   multiply f[r] = A[r][k] / pivot, r > k
//   update   A[r][c] = A[r][c] - f[r] * A[k][c], r > k, k < c <= S: a wave per row, its lanes along
//            the row with the pivot row's two elements in registers
//   back     k = S - 1 .. 0: x[k] = A[k][S] / D[k]; A[r][S] = A[r][S] - A[r][k] * x[k], r < k
//   norm     a = |x|; the squares padded with zeros to a power of two P and summed by the tree
//            v[i] += v[i + h], h = P / 2 .. 1; need = a / sqrt(sum)
// Degenerate (status 1, need = 1 / sqrt(S) in every component): a pivot that is exactly zero, or a
// result that is not finite.
#include "cobel_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxS = COBEL_PMA_MAX_STATES;
static_assert(kMaxS <= kThreads / 2, "the swap and the multipliers share one pass of the workgroup");

__host__ __device__ inline int need_ld(int S) { return (S + 1) | 1; }
__host__ __device__ inline int need_pow2(int S) {
  int p = 1;
  while (p < S) p *= 2;
  return p;
}
// A [S][ld], F [P] (multipliers, then the tree of squares), D [S] pivots, X [S] solution, one flag
size_t need_lds_bytes(int S) {
  return 8 * ((size_t)S * need_ld(S) + (size_t)need_pow2(S) + 2 * (size_t)S) + 8;
}

struct need_args {
  const double* T;          // [N][S][S]
  const int32_t* select;    // [N] or NULL
  double* need;             // [N][S]
  int32_t* status;          // [N]
  int32_t S;
};

__global__ __launch_bounds__(kThreads) void k_pma_stationary(const need_args P) {
  const int i = (int)blockIdx.x;
  if (P.select && P.select[i] >= 0) return;
  extern __shared__ __attribute__((aligned(16))) double need_lds[];
  const int S = P.S, ld = need_ld(S), P2 = need_pow2(S);
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  double* const A = need_lds;
  double* const F = A + (size_t)S * ld;
  double* const D = F + P2;
  double* const X = D + S;
  int* const flag = reinterpret_cast<int*>(X + S);
  const double w = 1.0 / (double)S;
  const double* const T = P.T + (size_t)i * S * S;
  // T is read along its rows, which are the columns of A
  for (int e = t; e < S * S; e += kThreads) {
    const int c = e / S, r = e - c * S;
    A[r * ld + c] = ((r == c ? 1.0 : 0.0) - T[e]) + w;
  }
  for (int r = t; r < S; r += kThreads) A[r * ld + S] = w;
  if (t == 0) *flag = 0;
  __syncthreads();

  bool zero = false;
  for (int k = 0; k < S; ++k) {
    // the pivot row (a value that is not a number never wins; if the column holds nothing else the
    // row is k, and the result is not finite)
    double bv = -1.0;
    int bi = k;
    for (int r = k + lane; r < S; r += 64) {
      const double v = fabs(A[r * ld + k]);
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
    const double pv = A[p * ld + k];
    if (pv == 0.0) {     // (the same for every lane of the workgroup)
      zero = true;
      break;
    }
    // lanes 0 .. 127 swap the rows past column k, lanes 128 .. 255 divide column k by the pivot
    if (t < kThreads / 2) {
      const int c = k + 1 + t;
      if (p != k && c <= S) {
        const double a = A[k * ld + c];
        A[k * ld + c] = A[p * ld + c];
        A[p * ld + c] = a;
      }
    } else {
      const int r = k + 1 + (t - kThreads / 2);
      if (r < S) F[r] = A[(r == p ? k : r) * ld + k] / pv;
      if (t == kThreads / 2) D[k] = pv;
    }
    __syncthreads();
    const int c0 = k + 1 + lane, c1 = c0 + 64;
    const double p0 = c0 <= S ? A[k * ld + c0] : 0.0;
    const double p1 = c1 <= S ? A[k * ld + c1] : 0.0;
    for (int r = k + 1 + wave; r < S; r += kWaves) {
      const double f = F[r];
      double* const row = A + r * ld;
      if (c0 <= S) row[c0] = row[c0] - f * p0;
      if (c1 <= S) row[c1] = row[c1] - f * p1;
    }
    __syncthreads();
  }

  double v = 0.0;
  if (!zero) {
    for (int k = S - 1; k >= 0; --k) {
      const double xk = A[k * ld + S] / D[k];
      if (t < k) A[t * ld + S] = A[t * ld + S] - A[t * ld + k] * xk;
      else if (t == k) X[k] = xk;
      __syncthreads();
    }
    const double a = t < S ? fabs(X[t]) : 0.0;
    if (t < P2) F[t] = a * a;
    __syncthreads();
    for (int h = P2 / 2; h >= 1; h >>= 1) {
      if (t < h) F[t] = F[t] + F[t + h];
      __syncthreads();
    }
    v = a / sqrt(F[0]);
    if (t < S && !__builtin_isfinite(v)) *flag = 1;
    __syncthreads();
  }
  const bool bad = zero || *flag != 0;
  if (t < S) P.need[(size_t)i * S + t] = bad ? 1.0 / sqrt((double)S) : v;
  if (t == 0) P.status[i] = bad ? 1 : 0;
}

}  // namespace

extern "C" int cobel_pma_plan_need(int32_t n_states, int32_t out[2]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_pma_plan_need: NULL out");
  out[0] = out[1] = 0;
  COBEL_REQUIRE(n_states >= 1 && n_states <= kMaxS, COBEL_E_UNSUPPORTED,
                "cobel_pma_plan_need: %d states (the stationary distribution is served for up to %d "
                "states)",
                n_states, kMaxS);
  out[0] = (int32_t)need_lds_bytes(n_states);
  out[1] = kThreads;
  return COBEL_OK;
}

extern "C" int cobel_pma_stationary(const cobel_pma_mem_t* mem, const int32_t* select, double* need,
                                    int32_t* status, void* stream) {
  COBEL_REQUIRE(mem, COBEL_E_ARG, "cobel_pma_stationary: NULL mem");
  COBEL_REQUIRE(!(mem->flags & COBEL_PMA_WIDE), COBEL_E_UNSUPPORTED,
                "cobel_pma_stationary: the wide form keeps compute_need(None) on the host (the "
                "kernel serves up to %d states, in LDS)",
                kMaxS);
  COBEL_REQUIRE(mem->n_states >= 1 && mem->n_states <= kMaxS, COBEL_E_UNSUPPORTED,
                "cobel_pma_stationary: %d states (the stationary distribution is served for up to "
                "%d states)",
                mem->n_states, kMaxS);
  COBEL_REQUIRE(mem->n >= 1, COBEL_E_RANGE, "cobel_pma_stationary: n = %d", mem->n);
  COBEL_REQUIRE(mem->T && need && status, COBEL_E_ARG,
                "cobel_pma_stationary: T, need and status are required");
  COBEL_REQUIRE((((uintptr_t)mem->T | (uintptr_t)need) & 7u) == 0 &&
                    (((uintptr_t)select | (uintptr_t)status) & 3u) == 0,
                COBEL_E_ARG, "cobel_pma_stationary: misaligned argument");
  need_args P;
  P.T = mem->T;
  P.select = select;
  P.need = need;
  P.status = status;
  P.S = mem->n_states;
  COBEL_HIP_TRY(cobel_launch(k_pma_stationary, dim3((unsigned)mem->n), dim3(kThreads),
                             need_lds_bytes(mem->n_states), (hipStream_t)stream, P));
  return COBEL_OK;
}
