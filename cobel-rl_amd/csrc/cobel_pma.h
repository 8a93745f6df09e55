// Device functions the PMA kernel files share (pma.hip: replay and trial; pma_gain.hip: the gain
// maps, n-step gains, action probabilities and update_q as calls of their own): rows of a float64
// Q table, NumPy's order of a row sum, and the gain of one backup.  One rounding per operation
// (-ffp-contract=off), as everywhere in these files.
#pragma once
#include "cobel_common.h"
#include "cobel_policy.h"

namespace {

constexpr int kMaxA = COBEL_PMA_MAX_ACTIONS;

// np.sum over a row of A values: a plain loop below eight, numpy's eight accumulators at eight
__device__ __forceinline__ double sum_row(const double (&v)[kMaxA], int A) {
  if (A == 8) return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  double r = 0.0 + v[0];
#pragma unroll
  for (int a = 1; a < kMaxA; ++a) r = a < A ? r + v[a] : r;
  return r;
}
__device__ __forceinline__ void load_row(const double* Q, int s, int A, double (&q)[kMaxA]) {
#pragma unroll
  for (int a = 0; a < kMaxA; ++a) q[a] = a < A ? Q[s * A + a] : 0.0;
}
// np.amax over a row
__device__ __forceinline__ double max_row(const double* Q, int s, int A) {
  double m = Q[s * A];
#pragma unroll
  for (int a = 1; a < kMaxA; ++a)
    if (a < A) {
      const double v = Q[s * A + a];
      m = v > m ? v : m;
    }
  return m;
}
// sum(q_new * p_new) - sum(q_new * p_old), the policies normalised (compute_gain_batch) or not
// (compute_gain)
__device__ __forceinline__ double policy_gain(const double (&q)[kMaxA], const double (&qn)[kMaxA],
                                              int A, uint32_t mask, double eps, bool normalise) {
  double po[kMaxA], pn[kMaxA];
  cobel_eps_greedy_select_n<double, kMaxA>(q, A, mask, 0.0, eps, po);
  cobel_eps_greedy_select_n<double, kMaxA>(qn, A, mask, 0.0, eps, pn);
#pragma unroll
  for (int a = 0; a < kMaxA; ++a) {
    if (a >= A) {
      po[a] = 0.0;
      pn[a] = 0.0;
    }
  }
  if (normalise) {
    const double so = sum_row(po, A), sn = sum_row(pn, A);
#pragma unroll
    for (int a = 0; a < kMaxA; ++a) {
      po[a] = po[a] / so;
      pn[a] = pn[a] / sn;
    }
  }
#pragma unroll
  for (int a = 0; a < kMaxA; ++a) {
    pn[a] = pn[a] * qn[a];
    po[a] = po[a] * qn[a];
  }
  return sum_row(pn, A) - sum_row(po, A);
}

}  // namespace
