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

// The parameters of one instance, staged once at the top of a kernel body (or of its loop over
// instances) and read from there: the launch's scalars, or, with cobel_pma_mem_sets_t.param_index, those
// of the instance's set and its rows of the two power tables.
// (the set is addressed through a pointer into global memory by its type: through a generic one,
//  as the copy of the by-value arguments is, the compiler would merge a scalar's two loads — from
//  the arguments, from the set — into one load through a selected pointer and copy the arguments
//  into scratch in every lane)
struct pma_par {
  double lr, lrq, lrT, gamma, gq, mg, eps;
  const double *gpow, *gqpow;
};
typedef const __attribute__((address_space(1))) cobel_pma_param_set_t* pma_set_ptr;
typedef const __attribute__((address_space(1))) uint16_t* pma_index_ptr;

// A value every lane of the wavefront holds alike, into scalar registers.  The instance is the
// workgroup's (or the wavefront's turn of a loop over instances), so its set is uniform; but a
// kernel that also stores cannot read it with scalar loads, and the doubles of a set would stay
// in vector registers for the length of the body.
__device__ __forceinline__ double pma_uniform(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the instance's set, or nullptr for a launch without sets; *row takes its index (an index past
// the table — a table edited by hand — is clamped to the last set, as load_tables clamps states)
__device__ __forceinline__ pma_set_ptr pma_set_of(const cobel_pma_mem_x& m, int i, int* row) {
  *row = 0;
  if (!m.param_index) return nullptr;
  int k = __builtin_amdgcn_readfirstlane((int)((pma_index_ptr)m.param_index)[i]);
  k = k < m.n_param_sets ? k : m.n_param_sets - 1;
  *row = k;
  return (pma_set_ptr)(m.param_sets + k);
}
// SETS = false: a kernel form that serves the scalar launch only and carries no code for sets
template <bool SETS>
__device__ __forceinline__ void pma_load_par(const cobel_pma_mem_x& m, int i, pma_par* p) {
  int row = 0;
  pma_set_ptr ps = nullptr;
  if constexpr (SETS) ps = pma_set_of(m, i, &row);
  p->lr = m.learning_rate;
  p->lrq = m.learning_rate_q;
  p->lrT = m.learning_rate_T;
  p->gamma = m.gamma;
  p->gq = m.gamma_q;
  p->mg = m.min_gain;
  p->eps = m.epsilon;
  p->gpow = m.gamma_pow;
  p->gqpow = m.gamma_q_pow;
  if (ps) {
    p->lr = pma_uniform(ps->learning_rate);
    p->lrq = pma_uniform(ps->learning_rate_q);
    p->lrT = pma_uniform(ps->learning_rate_T);
    p->gamma = pma_uniform(ps->gamma);
    p->gq = pma_uniform(ps->gamma_q);
    p->mg = pma_uniform(ps->min_gain);
    p->eps = pma_uniform(ps->epsilon);
    p->gpow = m.gamma_pow + (size_t)row * m.pow_len;
    p->gqpow = m.gamma_q_pow + (size_t)row * m.pow_len;
  }
}

// What every entry point that reads a parameter refuses of the sets before a launch: an index
// without sets, a count a 16-bit index cannot address, misaligned pointers.  Without an index the
// other two fields are not looked at.  (pow_len against the replay or sequence length is checked
// where that length is known; it holds for every row.)
inline int pma_check_sets(const cobel_pma_mem_x& m, const char* who) {
  if (!m.param_index) return COBEL_OK;
  COBEL_REQUIRE(m.param_sets, COBEL_E_ARG, "%s: param_index given without parameter sets", who);
  COBEL_REQUIRE(m.n_param_sets >= 1 && m.n_param_sets <= 65535, COBEL_E_ARG,
                "%s: %d parameter sets (1 ... 65535)", who, m.n_param_sets);
  COBEL_REQUIRE(((uintptr_t)m.param_sets & 15u) == 0 && ((uintptr_t)m.param_index & 1u) == 0,
                COBEL_E_ARG, "%s: param_sets must be 16-byte, param_index 2-byte aligned", who);
  return COBEL_OK;
}

}  // namespace
