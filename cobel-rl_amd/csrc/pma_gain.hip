// The observables of PMAMemory as device calls of their own: compute_gain_batch
// (cobel_pma_gain_batch), compute_gain (cobel_pma_gain_seq), action_probs_batch
// (cobel_pma_action_probs) and the n-step update_q (cobel_pma_update_q).  pma.hip's contract:
// float64 throughout, the reference's expression operation for operation, one rounding each
// (-ffp-contract=off), sums in NumPy's order (cobel_pma.h).  The expressions are those of
// pma_replay_body, which computes the same values every round and keeps only their arg-max.
//
// Every table is read in place from device memory: a gain map touches each entry once, so staging
// in LDS buys nothing, and one kernel serves the default and the wide form alike — no
// COBEL_PMA_WIDE branch and no LDS limit here; 1 .. COBEL_PMA_WIDE_MAX_STATES states,
// 1 .. COBEL_PMA_MAX_ACTIONS actions.  None of these kernels draws a number or moves a counter.
//
//   k_pma_gain_batch    one thread per backup a * S + s: consecutive threads take consecutive s for
//                       one a, so the Q rows coalesce; grid (ceil(A S / 256), instances)
//   k_pma_gain_seq      one wavefront per (instance, sequence): the lanes take the steps and leave
//                       the step gains in LDS, lane-uniform code adds them in sequence order
//   k_pma_action_probs  one thread per row
//   k_pma_update_q      one thread per instance: the bootstrap value first, then the steps in
//                       order, so a repeated (s, a) sees the earlier step's write
// With cobel_pma_mem_sets_t.param_index the gain kernels stage the instance's parameters (pma_load_par,
// cobel_pma.h) at the top of their loop over instances, and cobel_pma_update_q_sets runs
// k_pma_update_q's second form, which takes the learning rate and the row of powers of each
// instance's set.
//
// Reference behaviour restated (paths relative to the reference's src/cobel):
//   memory/pma.py:269-331 (compute_gain), :333-386 (compute_gain_batch), :423-450
//   (action_probs_batch), :452-496 (update_q); agent/pma.py:319-353 (update_q);
//   policy/greedy.py:77-86 (get_action_probs)
#include "cobel_common.h"
#include "cobel_pma.h"
#include "cobel_policy.h"

namespace {

constexpr int kMaxS = COBEL_PMA_WIDE_MAX_STATES;
constexpr int kMaxSeq = COBEL_PMA_MAX_SEQ;
constexpr int kThreads = 256;
constexpr unsigned kMaxGridY = 65535u;

struct gain_args {
  cobel_pma_mem_x m;
  const double* q;
  int64_t q_stride;
  double* gain;
};

struct seq_args {
  cobel_pma_mem_x m;
  const double* q;
  int64_t q_stride;
  const cobel_pma_rec_t* steps;
  const int32_t* lengths;
  int32_t n_seq, max_len;
  int64_t inst_stride;
  double* gain;
};

struct upd_args {
  double* q;
  const cobel_pma_rec_t* steps;
  const int32_t* lengths;
  const double* pow_table;
  int64_t inst_stride;
  double learning_rate;
  int32_t n, n_states, n_actions, max_len;
  // the form with sets: pow_table is [n_sets][pow_len], `agent` says which learning rate
  const cobel_pma_param_set_t* sets;
  const uint16_t* index;
  int32_t n_sets, pow_len, agent;
};

// (an index from a table or a record edited by hand must not send a row read outside the table)
__device__ __forceinline__ int clamp_to(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// memory/pma.py:333-386.  SETS: the form a launch with a param_index takes; the scalar launch keeps
// the form without a line of it (here the staging costs five vector registers, and with them a
// wave per SIMD).
template <bool SETS>
__global__ __launch_bounds__(kThreads) void k_pma_gain_batch(const gain_args P) {
  const cobel_pma_mem_x& m = P.m;
  const int S = m.n_states, A = m.n_actions, SA = S * A;
  const int idx = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (idx >= SA) return;
  const int a = idx / S, s = idx - a * S;
  const int c = s * A + a;
  const uint32_t mask = m.action_mask ? (uint32_t)m.action_mask[s] : 0xffu;
  for (int i = (int)blockIdx.y; i < m.n; i += (int)gridDim.y) {
    const double* const Q = P.q + (size_t)i * (size_t)P.q_stride;
    const size_t off = (size_t)i * SA;
    pma_par p;
    pma_load_par<SETS>(m, i, &p);
    double q[kMaxA], qn[kMaxA];
    load_row(Q, s, A, q);
    const double mx = max_row(Q, clamp_to(m.states[off + c], S), A);
    const double qa = Q[c];
    const double inner = (m.rewards[off + c] + (p.gq * mx) * (double)m.terminals[off + c]) - qa;
    const double qna = qa + p.lrq * inner;
#pragma unroll
    for (int b = 0; b < kMaxA; ++b) qn[b] = b == a ? qna : q[b];
    double gain = policy_gain(q, qn, A, mask, p.eps, true);
    gain = gain < p.mg ? p.mg : gain;
    P.gain[off + idx] = gain;
  }
}

// memory/pma.py:269-331, one update of the list per wavefront
template <bool SETS>
__global__ __launch_bounds__(64) void k_pma_gain_seq(const seq_args P) {
  __shared__ double sg[kMaxSeq], rr[kMaxSeq];
  const cobel_pma_mem_x& m = P.m;
  const int S = m.n_states, A = m.n_actions;
  const int lane = (int)threadIdx.x;
  const int k = (int)blockIdx.x;
  const bool original = m.flags & COBEL_PMA_GAIN_ORIGINAL;
  for (int i = (int)blockIdx.y; i < m.n; i += (int)gridDim.y) {
    const double* const Q = P.q + (size_t)i * (size_t)P.q_stride;
    pma_par p;
    pma_load_par<SETS>(m, i, &p);
    const cobel_pma_rec_t* const st =
        P.steps + (size_t)i * (size_t)P.inst_stride + (size_t)k * P.max_len;
    int n = P.lengths[(P.inst_stride ? (size_t)i * P.n_seq : 0) + k];
    n = n < 1 ? 1 : (n > P.max_len ? P.max_len : n);
    for (int j = lane; j < n; j += 64) rr[j] = st[j].reward;
    wsync();
    const double fv = max_row(Q, clamp_to(st[n - 1].next_state, S), A) * (double)st[n - 1].terminal;
    for (int j = lane; j < n; j += 64) {
      const int s = clamp_to(st[j].state, S), a = clamp_to(st[j].action, A);
      double r = 0.0;
      for (int kk = 0; kk < n - j; ++kk) r += rr[j + kk] * p.gpow[kk];
      const double tgt = r + fv * p.gqpow[n - j];
      double q[kMaxA], qn[kMaxA];
      load_row(Q, s, A, q);
#pragma unroll
      for (int b = 0; b < kMaxA; ++b) qn[b] = q[b] + p.lrq * ((b == a ? tgt : q[b]) - q[b]);
      const uint32_t mask = m.action_mask ? (uint32_t)m.action_mask[s] : 0xffu;
      double sgn = policy_gain(q, qn, A, mask, p.eps, false);
      if (original) sgn = p.mg > sgn ? p.mg : sgn;
      sg[j] = sgn;
    }
    wsync();
    double gain = 0.0;
    for (int j = 0; j < n; ++j) gain += sg[j];
    gain = p.mg > gain ? p.mg : gain;
    if (lane == 0) P.gain[(size_t)i * P.n_seq + k] = gain;
    wsync();
  }
}

// memory/pma.py:423-450
__global__ __launch_bounds__(kThreads) void k_pma_action_probs(const double* __restrict__ q,
                                                               const uint8_t* __restrict__ mask_bits,
                                                               int64_t rows, int32_t A, double eps,
                                                               double* __restrict__ probs) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
  if (r >= rows) return;
  double v[kMaxA], p[kMaxA];
  load_row(q + (size_t)r * A, 0, A, v);
  const uint32_t mask = mask_bits ? (uint32_t)mask_bits[r] : 0xffu;
  cobel_eps_greedy_select_n<double, kMaxA>(v, A, mask, 0.0, eps, p);
#pragma unroll
  for (int a = 0; a < kMaxA; ++a)
    if (a >= A) p[a] = 0.0;
  const double total = sum_row(p, A);
  double* const out = probs + (size_t)r * A;
#pragma unroll
  for (int a = 0; a < kMaxA; ++a)
    if (a < A) out[a] = p[a] / total;
}

// memory/pma.py:452-496 and agent/pma.py:319-353, which differ in the learning rate and the powers
// SETS: the learning rate and the row of powers of the instance's parameter set
template <bool SETS>
__global__ __launch_bounds__(64) void k_pma_update_q(const upd_args P) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= P.n) return;
  const int S = P.n_states, A = P.n_actions;
  double lr = P.learning_rate;
  const double* pow_table = P.pow_table;
  if constexpr (SETS) {
    int k = (int)((pma_index_ptr)P.index)[i];
    k = k < P.n_sets ? k : P.n_sets - 1;
    const pma_set_ptr ps = (pma_set_ptr)(P.sets + k);
    lr = P.agent ? ps->alpha : ps->learning_rate_q;
    pow_table = P.pow_table + (size_t)k * P.pow_len;
  }
  double* const Q = P.q + (size_t)i * S * A;
  const cobel_pma_rec_t* const st = P.steps + (size_t)i * (size_t)P.inst_stride;
  int n = P.lengths[P.inst_stride ? i : 0];
  n = n < 1 ? 1 : (n > P.max_len ? P.max_len : n);
  // a step other than the last that finds terminal == 0 at or after itself ends the update
  // (:476-489): the first step looks at every step, so nothing is written at all
  if (n > 1)
    for (int j = 0; j < n; ++j)
      if (st[j].terminal == 0) return;
  const double fv = max_row(Q, clamp_to(st[n - 1].next_state, S), A) * (double)st[n - 1].terminal;
  for (int j = 0; j < n; ++j) {
    double r = 0.0;
    for (int kk = 0; kk < n - j; ++kk) r += st[j + kk].reward * pow_table[kk];
    const int cell = clamp_to(st[j].state, S) * A + clamp_to(st[j].action, A);
    const double qv = Q[cell];
    double td = r + fv * pow_table[n - j];
    td -= qv;
    Q[cell] = qv + lr * td;
  }
}

// what the four calls ask of the memory: its shape, and the tables `tables` says they read
int check_shape(const cobel_pma_mem_x* mem, const char* who) {
  COBEL_REQUIRE(mem, COBEL_E_ARG, "%s: NULL mem", who);
  COBEL_REQUIRE(mem->n_states >= 1 && mem->n_states <= kMaxS && mem->n_actions >= 1 &&
                    mem->n_actions <= kMaxA,
                COBEL_E_UNSUPPORTED,
                "%s: %d states, %d actions (this call serves 1 .. %d states and 1 .. %d actions)",
                who, mem->n_states, mem->n_actions, kMaxS, kMaxA);
  COBEL_REQUIRE(mem->n >= 0, COBEL_E_RANGE, "%s: n = %d", who, mem->n);
  return COBEL_OK;
}

int check_gain(const cobel_pma_mem_x* mem, const double* q, int64_t q_stride, const double* gain,
               const char* who) {
  if (int rc = check_shape(mem, who)) return rc;
  const cobel_pma_mem_x& m = *mem;
  COBEL_REQUIRE(q, COBEL_E_ARG, "%s: NULL q", who);
  COBEL_REQUIRE(gain, COBEL_E_ARG, "%s: NULL gain", who);
  COBEL_REQUIRE(m.rewards && m.states && m.terminals, COBEL_E_ARG,
                "%s: rewards, states and terminals are required", who);
  COBEL_REQUIRE(q_stride == 0 || q_stride == (int64_t)m.n_states * m.n_actions, COBEL_E_ARG,
                "%s: q_stride = %lld (0: one table for every instance, or %d)", who,
                (long long)q_stride, m.n_states * m.n_actions);
  COBEL_REQUIRE((((uintptr_t)q | (uintptr_t)gain | (uintptr_t)m.rewards) & 7u) == 0 &&
                    (((uintptr_t)m.states | (uintptr_t)m.terminals) & 3u) == 0,
                COBEL_E_ARG, "%s: misaligned table", who);
  // (with an index the scalars are ignored; a set's epsilon is checked where the set is filled)
  COBEL_REQUIRE(m.param_index || (m.epsilon >= 0.0 && m.epsilon <= 1.0), COBEL_E_ARG,
                "%s: epsilon %g outside [0, 1]", who, m.epsilon);
  return pma_check_sets(m, who);
}

// lengths [host] [count]: each 1 .. max_len; *longest takes the largest
int check_lengths(const int32_t* lengths, int64_t count, int32_t max_len, const char* who,
                  int32_t* longest) {
  COBEL_REQUIRE(lengths, COBEL_E_ARG, "%s: NULL lengths", who);
  *longest = 0;
  for (int64_t k = 0; k < count; ++k) {
    COBEL_REQUIRE(lengths[k] >= 1 && lengths[k] <= max_len, COBEL_E_RANGE,
                  "%s: lengths[%lld] = %d outside 1 .. max_len = %d", who, (long long)k, lengths[k],
                  max_len);
    *longest = lengths[k] > *longest ? lengths[k] : *longest;
  }
  return COBEL_OK;
}

// The lengths are host memory (they are checked before anything is launched); the kernel reads a
// copy whose allocation, filling and release are ordered by the stream.
struct device_lengths {
  int32_t* ptr = nullptr;
  hipStream_t st;
  explicit device_lengths(hipStream_t s) : st(s) {}
  hipError_t upload(const int32_t* host, size_t count) {
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&ptr), count * sizeof(int32_t), st);
    if (e != hipSuccess) {
      ptr = nullptr;
      return e;
    }
    return hipMemcpyAsync(ptr, host, count * sizeof(int32_t), hipMemcpyHostToDevice, st);
  }
  ~device_lengths() {
    if (ptr) (void)hipFreeAsync(ptr, st);
  }
};

unsigned grid_y(int n) { return (unsigned)n < kMaxGridY ? (unsigned)n : kMaxGridY; }

}  // namespace

extern "C" int cobel_pma_gain_batch(const cobel_pma_mem_t* mem_in, const double* q, int64_t q_stride,
                                    double* gain, void* stream) {
  COBEL_PMA_MEM("cobel_pma_gain_batch");
  if (int rc = check_gain(mem, q, q_stride, gain, "cobel_pma_gain_batch")) return rc;
  if (mem->n == 0) return COBEL_OK;
  gain_args P;
  P.m = *mem;
  P.q = q;
  P.q_stride = q_stride;
  P.gain = gain;
  const int SA = mem->n_states * mem->n_actions;
  COBEL_HIP_TRY(cobel_launch(mem->param_index ? k_pma_gain_batch<true> : k_pma_gain_batch<false>,
                             dim3((unsigned)((SA + kThreads - 1) / kThreads), grid_y(mem->n)),
                             dim3(kThreads), 0, (hipStream_t)stream, P));
  return COBEL_OK;
}

extern "C" int cobel_pma_gain_seq(const cobel_pma_mem_t* mem_in, const double* q, int64_t q_stride,
                                  const cobel_pma_rec_t* steps, const int32_t* lengths,
                                  int32_t n_seq, int32_t max_len, int64_t inst_stride, double* gain,
                                  void* stream) {
  const char* const who = "cobel_pma_gain_seq";
  COBEL_PMA_MEM(who);
  if (int rc = check_gain(mem, q, q_stride, gain, who)) return rc;
  COBEL_REQUIRE(n_seq >= 0, COBEL_E_RANGE, "%s: n_seq = %d", who, n_seq);
  if (n_seq == 0 || mem->n == 0) return COBEL_OK;
  COBEL_REQUIRE(steps && ((uintptr_t)steps & 7u) == 0, COBEL_E_ARG,
                "%s: steps must be given, 8-byte aligned", who);
  COBEL_REQUIRE(max_len >= 1 && max_len <= kMaxSeq, COBEL_E_UNSUPPORTED,
                "%s: max_len = %d (sequences of 1 .. %d steps are served)", who, max_len, kMaxSeq);
  COBEL_REQUIRE(inst_stride == 0 || inst_stride == (int64_t)n_seq * max_len, COBEL_E_ARG,
                "%s: inst_stride = %lld (0: one list for every instance, or n_seq * max_len = %lld)",
                who, (long long)inst_stride, (long long)n_seq * max_len);
  const int64_t count = (int64_t)n_seq * (inst_stride ? mem->n : 1);
  int32_t longest = 0;
  if (int rc = check_lengths(lengths, count, max_len, who, &longest)) return rc;
  COBEL_REQUIRE(mem->gamma_pow && mem->gamma_q_pow &&
                    (((uintptr_t)mem->gamma_pow | (uintptr_t)mem->gamma_q_pow) & 7u) == 0,
                COBEL_E_ARG, "%s: the two power tables are required, 8-byte aligned", who);
  COBEL_REQUIRE(mem->pow_len > longest, COBEL_E_ARG,
                "%s: the power tables hold %d entries, %d are needed", who, mem->pow_len,
                longest + 1);
  device_lengths dl((hipStream_t)stream);
  COBEL_HIP_TRY(dl.upload(lengths, (size_t)count));
  seq_args P;
  P.m = *mem;
  P.q = q;
  P.q_stride = q_stride;
  P.steps = steps;
  P.lengths = dl.ptr;
  P.n_seq = n_seq;
  P.max_len = max_len;
  P.inst_stride = inst_stride;
  P.gain = gain;
  COBEL_HIP_TRY(cobel_launch(mem->param_index ? k_pma_gain_seq<true> : k_pma_gain_seq<false>,
                             dim3((unsigned)n_seq, grid_y(mem->n)), dim3(64), 0, (hipStream_t)stream,
                             P));
  return COBEL_OK;
}

extern "C" int cobel_pma_action_probs(const double* q, const uint8_t* mask_bits, int64_t rows,
                                      int32_t n_actions, double epsilon, double* probs,
                                      void* stream) {
  const char* const who = "cobel_pma_action_probs";
  COBEL_REQUIRE(q, COBEL_E_ARG, "%s: NULL q", who);
  COBEL_REQUIRE(probs, COBEL_E_ARG, "%s: NULL probs", who);
  COBEL_REQUIRE(n_actions >= 1 && n_actions <= kMaxA, COBEL_E_UNSUPPORTED,
                "%s: %d actions (this call serves 1 .. %d actions)", who, n_actions, kMaxA);
  COBEL_REQUIRE(rows >= 0 && rows <= (int64_t)0x7fffffff * kThreads, COBEL_E_RANGE,
                "%s: rows = %lld", who, (long long)rows);
  COBEL_REQUIRE((((uintptr_t)q | (uintptr_t)probs) & 7u) == 0, COBEL_E_ARG, "%s: misaligned table",
                who);
  COBEL_REQUIRE(epsilon >= 0.0 && epsilon <= 1.0, COBEL_E_ARG, "%s: epsilon %g outside [0, 1]", who,
                epsilon);
  if (rows == 0) return COBEL_OK;
  hipLaunchKernelGGL(k_pma_action_probs, dim3((unsigned)((rows + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, (hipStream_t)stream, q, mask_bits, rows, n_actions, epsilon,
                     probs);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

// both forms of the update: the checks, the lengths' copy, the launch
static int update_q_call(const char* who, const cobel_pma_mem_t* mem_in, double* q,
                         const cobel_pma_rec_t* steps, const int32_t* lengths, int32_t max_len,
                         int64_t inst_stride, double learning_rate, const double* pow_table,
                         int32_t pow_len, bool sets, int32_t agent, void* stream) {
  COBEL_PMA_MEM(who);
  if (int rc = check_shape(mem, who)) return rc;
  if (sets) {
    COBEL_REQUIRE(mem->param_index, COBEL_E_ARG, "%s: the memory carries no param_index", who);
    if (int rc = pma_check_sets(*mem, who)) return rc;
    COBEL_REQUIRE(agent == COBEL_PMA_Q_MEMORY || agent == COBEL_PMA_Q_AGENT, COBEL_E_ARG,
                  "%s: which = %d (COBEL_PMA_Q_MEMORY or COBEL_PMA_Q_AGENT)", who, agent);
  }
  COBEL_REQUIRE(q && ((uintptr_t)q & 7u) == 0, COBEL_E_ARG, "%s: NULL q, or not 8-byte aligned", who);
  COBEL_REQUIRE(steps && ((uintptr_t)steps & 7u) == 0, COBEL_E_ARG,
                "%s: steps must be given, 8-byte aligned", who);
  COBEL_REQUIRE(max_len >= 1 && max_len <= kMaxSeq, COBEL_E_UNSUPPORTED,
                "%s: max_len = %d (sequences of 1 .. %d steps are served)", who, max_len, kMaxSeq);
  COBEL_REQUIRE(inst_stride == 0 || inst_stride == (int64_t)max_len, COBEL_E_ARG,
                "%s: inst_stride = %lld (0: one sequence for every instance, or max_len = %d)", who,
                (long long)inst_stride, max_len);
  const int64_t count = inst_stride ? mem->n : 1;
  int32_t longest = 0;
  if (int rc = check_lengths(lengths, count, max_len, who, &longest)) return rc;
  COBEL_REQUIRE(pow_table && ((uintptr_t)pow_table & 7u) == 0, COBEL_E_ARG,
                "%s: the power table is required, 8-byte aligned", who);
  COBEL_REQUIRE(pow_len > longest, COBEL_E_ARG, "%s: the power table holds %d entries, %d are needed",
                who, pow_len, longest + 1);
  if (mem->n == 0) return COBEL_OK;
  device_lengths dl((hipStream_t)stream);
  COBEL_HIP_TRY(dl.upload(lengths, (size_t)count));
  upd_args P;
  P.q = q;
  P.steps = steps;
  P.lengths = dl.ptr;
  P.pow_table = pow_table;
  P.inst_stride = inst_stride;
  P.learning_rate = learning_rate;
  P.n = mem->n;
  P.n_states = mem->n_states;
  P.n_actions = mem->n_actions;
  P.max_len = max_len;
  P.sets = sets ? mem->param_sets : nullptr;
  P.index = sets ? mem->param_index : nullptr;
  P.n_sets = sets ? mem->n_param_sets : 0;
  P.pow_len = pow_len;
  P.agent = agent;
  COBEL_HIP_TRY(cobel_launch(sets ? k_pma_update_q<true> : k_pma_update_q<false>,
                             dim3((unsigned)((mem->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                             P));
  return COBEL_OK;
}

extern "C" int cobel_pma_update_q(const cobel_pma_mem_t* mem, double* q,
                                  const cobel_pma_rec_t* steps, const int32_t* lengths,
                                  int32_t max_len, int64_t inst_stride, double learning_rate,
                                  const double* pow_table, int32_t pow_len, void* stream) {
  return update_q_call("cobel_pma_update_q", mem, q, steps, lengths, max_len, inst_stride,
                       learning_rate, pow_table, pow_len, false, 0, stream);
}

extern "C" int cobel_pma_update_q_sets(const cobel_pma_mem_t* mem, double* q,
                                       const cobel_pma_rec_t* steps, const int32_t* lengths,
                                       int32_t max_len, int64_t inst_stride, int32_t which,
                                       const double* agent_pow, void* stream) {
  const char* const who = "cobel_pma_update_q_sets";
  COBEL_REQUIRE(mem, COBEL_E_ARG, "%s: NULL mem", who);
  const double* const table = which == COBEL_PMA_Q_AGENT ? agent_pow : mem->gamma_q_pow;
  return update_q_call(who, mem, q, steps, lengths, max_len, inst_stride, 0.0, table, mem->pow_len,
                       true, which, stream);
}
