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
  cobel_pma_mem_t m;
  const double* q;
  int64_t q_stride;
  double* gain;
};

struct seq_args {
  cobel_pma_mem_t m;
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
};

// (an index from a table or a record edited by hand must not send a row read outside the table)
__device__ __forceinline__ int clamp_to(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// memory/pma.py:333-386
__global__ __launch_bounds__(kThreads) void k_pma_gain_batch(const gain_args P) {
  const cobel_pma_mem_t& m = P.m;
  const int S = m.n_states, A = m.n_actions, SA = S * A;
  const int idx = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (idx >= SA) return;
  const int a = idx / S, s = idx - a * S;
  const int c = s * A + a;
  const uint32_t mask = m.action_mask ? (uint32_t)m.action_mask[s] : 0xffu;
  for (int i = (int)blockIdx.y; i < m.n; i += (int)gridDim.y) {
    const double* const Q = P.q + (size_t)i * (size_t)P.q_stride;
    const size_t off = (size_t)i * SA;
    double q[kMaxA], qn[kMaxA];
    load_row(Q, s, A, q);
    const double mx = max_row(Q, clamp_to(m.states[off + c], S), A);
    const double qa = Q[c];
    const double inner = (m.rewards[off + c] + (m.gamma_q * mx) * (double)m.terminals[off + c]) - qa;
    const double qna = qa + m.learning_rate_q * inner;
#pragma unroll
    for (int b = 0; b < kMaxA; ++b) qn[b] = b == a ? qna : q[b];
    double gain = policy_gain(q, qn, A, mask, m.epsilon, true);
    gain = gain < m.min_gain ? m.min_gain : gain;
    P.gain[off + idx] = gain;
  }
}

// memory/pma.py:269-331, one update of the list per wavefront
__global__ __launch_bounds__(64) void k_pma_gain_seq(const seq_args P) {
  __shared__ double sg[kMaxSeq], rr[kMaxSeq];
  const cobel_pma_mem_t& m = P.m;
  const int S = m.n_states, A = m.n_actions;
  const int lane = (int)threadIdx.x;
  const int k = (int)blockIdx.x;
  const bool original = m.flags & COBEL_PMA_GAIN_ORIGINAL;
  for (int i = (int)blockIdx.y; i < m.n; i += (int)gridDim.y) {
    const double* const Q = P.q + (size_t)i * (size_t)P.q_stride;
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
      for (int kk = 0; kk < n - j; ++kk) r += rr[j + kk] * m.gamma_pow[kk];
      const double tgt = r + fv * m.gamma_q_pow[n - j];
      double q[kMaxA], qn[kMaxA];
      load_row(Q, s, A, q);
#pragma unroll
      for (int b = 0; b < kMaxA; ++b) qn[b] = q[b] + m.learning_rate_q * ((b == a ? tgt : q[b]) - q[b]);
      const uint32_t mask = m.action_mask ? (uint32_t)m.action_mask[s] : 0xffu;
      double sgn = policy_gain(q, qn, A, mask, m.epsilon, false);
      if (original) sgn = m.min_gain > sgn ? m.min_gain : sgn;
      sg[j] = sgn;
    }
    wsync();
    double gain = 0.0;
    for (int j = 0; j < n; ++j) gain += sg[j];
    gain = m.min_gain > gain ? m.min_gain : gain;
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
__global__ __launch_bounds__(64) void k_pma_update_q(const upd_args P) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= P.n) return;
  const int S = P.n_states, A = P.n_actions;
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
    for (int kk = 0; kk < n - j; ++kk) r += st[j + kk].reward * P.pow_table[kk];
    const int cell = clamp_to(st[j].state, S) * A + clamp_to(st[j].action, A);
    const double qv = Q[cell];
    double td = r + fv * P.pow_table[n - j];
    td -= qv;
    Q[cell] = qv + P.learning_rate * td;
  }
}

// what the four calls ask of the memory: its shape, and the tables `tables` says they read
int check_shape(const cobel_pma_mem_t* mem, const char* who) {
  COBEL_REQUIRE(mem, COBEL_E_ARG, "%s: NULL mem", who);
  COBEL_REQUIRE(mem->n_states >= 1 && mem->n_states <= kMaxS && mem->n_actions >= 1 &&
                    mem->n_actions <= kMaxA,
                COBEL_E_UNSUPPORTED,
                "%s: %d states, %d actions (this call serves 1 .. %d states and 1 .. %d actions)",
                who, mem->n_states, mem->n_actions, kMaxS, kMaxA);
  COBEL_REQUIRE(mem->n >= 0, COBEL_E_RANGE, "%s: n = %d", who, mem->n);
  return COBEL_OK;
}

int check_gain(const cobel_pma_mem_t* mem, const double* q, int64_t q_stride, const double* gain,
               const char* who) {
  if (int rc = check_shape(mem, who)) return rc;
  const cobel_pma_mem_t& m = *mem;
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
  COBEL_REQUIRE(m.epsilon >= 0.0 && m.epsilon <= 1.0, COBEL_E_ARG, "%s: epsilon %g outside [0, 1]",
                who, m.epsilon);
  return COBEL_OK;
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

extern "C" int cobel_pma_gain_batch(const cobel_pma_mem_t* mem, const double* q, int64_t q_stride,
                                    double* gain, void* stream) {
  if (int rc = check_gain(mem, q, q_stride, gain, "cobel_pma_gain_batch")) return rc;
  if (mem->n == 0) return COBEL_OK;
  gain_args P;
  P.m = *mem;
  P.q = q;
  P.q_stride = q_stride;
  P.gain = gain;
  const int SA = mem->n_states * mem->n_actions;
  COBEL_HIP_TRY(cobel_launch(k_pma_gain_batch,
                             dim3((unsigned)((SA + kThreads - 1) / kThreads), grid_y(mem->n)),
                             dim3(kThreads), 0, (hipStream_t)stream, P));
  return COBEL_OK;
}

extern "C" int cobel_pma_gain_seq(const cobel_pma_mem_t* mem, const double* q, int64_t q_stride,
                                  const cobel_pma_rec_t* steps, const int32_t* lengths,
                                  int32_t n_seq, int32_t max_len, int64_t inst_stride, double* gain,
                                  void* stream) {
  const char* const who = "cobel_pma_gain_seq";
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
  COBEL_HIP_TRY(cobel_launch(k_pma_gain_seq, dim3((unsigned)n_seq, grid_y(mem->n)), dim3(64), 0,
                             (hipStream_t)stream, P));
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

extern "C" int cobel_pma_update_q(const cobel_pma_mem_t* mem, double* q,
                                  const cobel_pma_rec_t* steps, const int32_t* lengths,
                                  int32_t max_len, int64_t inst_stride, double learning_rate,
                                  const double* pow_table, int32_t pow_len, void* stream) {
  const char* const who = "cobel_pma_update_q";
  if (int rc = check_shape(mem, who)) return rc;
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
  COBEL_HIP_TRY(cobel_launch(k_pma_update_q, dim3((unsigned)((mem->n + 63) / 64)), dim3(64), 0,
                             (hipStream_t)stream, P));
  return COBEL_OK;
}
