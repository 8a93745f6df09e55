// QAgent on a Sequence environment (agent/q.py, interface/sequence.py, policy/softmax.py and
// policy/greedy.py of the reference): the trial loops of a whole session in one launch — action
// selection, the Sequence step, the experience log, update_q and the replay batch of every step.
//
// Packing.  An instance takes a group of eight lanes, lane a holding the column of action a (lanes
// beyond n_actions carry -inf into a maximum, +0.0 into a sum, and store nothing); a wavefront holds
// eight instances, a workgroup kWaves wavefronts.  The instance's Q table [n_keys][n_actions] lives
// in LDS for the launch and is written back at its end.  The tables of the instances of a workgroup
// lie `stride` doubles apart, stride = 8 mod 32: the 64-byte rows the four groups of a 32-lane half
// read at one key then fall on four different quarters of the 256-byte bank row.  A group touches
// its own table only and all its lanes sit in one wavefront, so LDS traffic is ordered by wsync()
// alone, without a barrier.
//
// Order of the arithmetic (every lane of a group ends with the same bits, nothing is broadcast):
//   row maximum        a butterfly over the eight lanes (a maximum does not depend on the order)
//   softmax            e_a = exp((v_a - max) * beta), the A exponentials side by side;
//                      sum = ((e_0 + e_1) + e_2) + ... in action order, p_a = e_a / sum;
//                      cum_a = ((p_0 + p_1) + ...) + p_a, action = #{a < A - 1 : cum_a / cum_{A-1} <= u}
//   update_q           td = r; td += (gamma * nonterminal) * max(Q[next]); td -= Q[s][a];
//                      Q[s][a] += lr * td — each operation rounded (the file is compiled with
//                      -ffp-contract=off)
// A NaN in Q is not carried through the maxima as np.amax would carry it.
//
// Replay.  Only the B updates of a batch depend on one another; its B indices depend on len(M)
// alone.  So the lanes of a group evaluate the Philox blocks of eight indices side by side and
// gather the eight records, kChunk = 32 of them (four rounds) before the chain of updates starts;
// the chain takes the records from registers.  Batches beyond 32 repeat that: the log does not
// change while a batch is replayed.
//
// Why a gather cannot see a stale record.  A replay index may name a record the group wrote earlier
// in this launch, in a cache line a lane has already read.  (1) The record of the current step is
// never read back: it is forwarded from registers.  (2) Older records were stored by the same
// wavefront at least one step ago, and every step with a batch waits for its gathered loads
// (s_waitcnt vmcnt(0): on gfx9 the counter covers the wavefront's stores too, and they retire in
// order), so those stores have reached the L2 before any later gather is issued; without a batch
// nothing is gathered before the launch ends.  (3) The gather loads are relaxed agent-scope atomic
// loads (global_load ... sc1): they are served by the L2, where the stores landed, and not by a
// line the CU's vector cache kept from an earlier gather.  The workgroup stays on one XCD, so one L2
// sees both.
//
// The td a step reports is that of the last update of the step's own experience: the online one,
// or a replay of it in the same step's batch.
//
// Instances of one wavefront may follow schedules of different trial lengths: the loop runs while
// any lane is alive, shuffles stay in wave-uniform control flow, and everything an instance does is
// predicated on its own `alive`.  Table indices are clamped before use.
#include "cobel_seq.h"

#include "cobel_policy.h"

namespace {

using namespace cobel_seq;

constexpr int kG = 8;                          // lanes per instance
constexpr int kPerWave = 64 / kG;              // instances per wavefront
constexpr int kPerBlock = kWaves * kPerWave;   // ... per workgroup
constexpr int kRounds = 4;                     // gather rounds before a chain of updates
constexpr int kChunk = kRounds * kG;

static_assert(sizeof(cobel_qseq_rec_t) == 16, "a logged experience takes 16 bytes");
static_assert(kG == COBEL_QSEQ_MAX_ACTIONS, "one lane per action");

// doubles between the tables of two instances in LDS: the smallest count >= n_keys * A that is
// 8 mod 32 (64 bytes mod 256)
inline int q_stride(int n_keys, int A) {
  int s = n_keys * A;
  while ((s & 31) != 8) ++s;
  return s;
}

__device__ __forceinline__ double gmax(double v) {
#pragma unroll
  for (int o = 1; o < kG; o <<= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// The popcount of `pass` over the lanes of this lane's group
__device__ __forceinline__ int gcount(bool pass, int lane) {
  const unsigned long long b = __ballot(pass);
  return __popc((uint32_t)(b >> (lane & ~(kG - 1))) & 0xffu);
}

// Softmax.get_action_probs and the Generator.choice draw (see the head of the file).  v: the value
// of action a (this lane's); allowed: bit k set = action k takes part; p: this lane's probability.
// To be called in wave-uniform control flow.
__device__ __forceinline__ int softmax_group(double v, int a, int A, uint32_t allowed, double beta,
                                             double u, int lane, double& p) {
  const bool on = a < A && ((allowed >> a) & 1u);
  const double m = gmax(on ? v : -__builtin_huge_val());
  const double e = on ? exp((v - m) * beta) : 0.0;
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < kG; ++k) sum = sum + __shfl(e, k, kG);
  p = on ? e / sum : 0.0;
  double run = 0.0, cum = 0.0, total = 0.0;
#pragma unroll
  for (int k = 0; k < kG; ++k) {
    const double pk = __shfl(p, k, kG);
    run = (k == 0) ? pk : run + pk;
    cum = (k == a) ? run : cum;
    total = (k == A - 1) ? run : total;
  }
  return gcount(a < A - 1 && cum / total <= u, lane);
}

// update_q (agent/q.py:304-313) on the group's table; returns td.  `on`: the instance learns.
__device__ __forceinline__ double update_q(double* q, int A, int a, int s, int act, double r, int ns,
                                           int nt, double lr, double gamma, bool on) {
  const double qn = a < A ? q[ns * A + a] : -__builtin_huge_val();
  const double mx = gmax(qn);
  const double qsa = q[s * A + act];
  double td = r;
  td = td + (gamma * (double)nt) * mx;
  td = td - qsa;
  if (on && a == act) q[s * A + act] = qsa + lr * td;
  wsync();
  return td;
}

struct qseq_args {
  cobel_seq_t s;
  cobel_qseq_run_t r;
  int stride;
};

__global__ __launch_bounds__(64 * kWaves) void k_qseq_run(const qseq_args K) {
  extern __shared__ double lds_q[];
  const cobel_seq_t& S = K.s;
  const cobel_qseq_run_t& R = K.r;
  const int A = R.n_actions, NK = R.n_keys, B = R.batch_size;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int a = lane & (kG - 1);
  const int slot = wave * kPerWave + lane / kG;
  const long long inst = (long long)blockIdx.x * kPerBlock + slot;
  const bool valid = inst < (long long)S.n;
  const int i = valid ? (int)inst : 0;
  const bool mine = valid && a < A;      // this lane holds a column
  const bool head = valid && a == 0;     // ... and writes what the instance has one of
  const bool learn = R.flags & COBEL_F_LEARN;
  const uint32_t g = R.instance_ids ? R.instance_ids[i] : R.instance_base + (uint32_t)i;
  double* const q = lds_q + (size_t)slot * K.stride;

  for (int k = 0; k < NK; ++k)
    if (a < A) q[k * A + a] = valid ? R.Q[((size_t)i * NK + k) * A + a] : 0.0;
  wsync();

  const double* const pp = R.par + (size_t)(R.par_rows > 1 ? i : 0) * 4;
  const double lr = pp[0], gamma = pp[1], p_pol = pp[2];
  const int32_t* const toff = trial_offsets(S, i);
  const int cap = R.log_cap;
  cobel_qseq_rec_t* const rlog = learn ? R.log + (size_t)i * cap : nullptr;

  int ct = S.cur_trial[i], cs = S.cur_step[i];
  bool mid = R.mid[i] != 0;
  double trew = R.trew[i];
  uint32_t cp = R.pol_ctr[i];
  uint32_t cm = learn ? R.mem_ctr[i] : 0u;
  uint32_t loglen = learn ? min((uint32_t)R.log_len[i], (uint32_t)cap) : 0u;
  int done = 0, last_action = 0;
  long long budget = R.step_budget > 0 ? (long long)R.step_budget : 0x7fffffffffffffffll;
  unsigned long long executed = 0;
  int row = (R.trace && valid) ? max(R.trace_len[i], 0) : 0;
  bool alive = valid && R.trials > 0;
  int l_s = 0, l_ns = 0, l_nt = 0;
  double l_r = 0.0, l_td = 0.0;

  while (__ballot(alive) != 0ull) {
    if (alive && !mid) {   // Sequence.reset (interface/sequence.py:188-204)
      cs = 0;
      trew = 0.0;
      mid = true;
    }
    int base, len;
    const int at = step_at(S, toff, ct, cs, base, len);
    const int oi = clampi(S.step_obs[at], 0, S.n_obs - 1);
    const int s = clampi(R.key_of_row[oi], 0, NK - 1);
    // select_action on Q[state] (agent/q.py:199, :263)
    const double v = a < A ? q[s * A + a] : 0.0;
    const double u = cobel_draw_u01(cp, 0u, g, R.pol_stream, R.seed);
    if (alive) cp += 1u;
    int action;
    if (R.policy == COBEL_QSEQ_POLICY_SOFTMAX) {
      double p;
      action = softmax_group(v, a, A, 0xffu, p_pol, u, lane, p);
    } else {
      double row_v[kG];
#pragma unroll
      for (int k = 0; k < kG; ++k) row_v[k] = __shfl(v, k, kG);
      action = cobel_eps_greedy_select_n<double, kG>(row_v, A, 0xffu, u, p_pol, nullptr);
    }
    action = clampi(action, 0, A - 1);
    // Sequence.step (interface/sequence.py:129-186)
    const double reward = step_reward(S, at, action);
    const bool end = cs + 1 >= len;
    const int nx = clampi(base + clampi(cs + 1, 0, len - 1), 0, S.n_steps - 1);
    const int noi = end ? 0 : clampi(S.step_obs[nx], 0, S.n_obs - 1);
    const int ns = clampi(R.key_of_row[noi], 0, NK - 1);
    const int nt = end ? 0 : 1;
    double td = 0.0;
    if (learn) {
      // M.append(experience) (agent/q.py:213); a full log takes no record
      const uint32_t meta = (uint32_t)s | ((uint32_t)ns << 8) | ((uint32_t)action << 16) |
                            ((uint32_t)nt << 24);
      const bool appended = alive && loglen < (uint32_t)cap;
      if (head && appended) {
        cobel_qseq_rec_t rec;
        rec.reward = reward;
        rec.meta = meta;
        rec.reserved_ = 0u;
        rlog[loglen] = rec;
      }
      if (appended) loglen += 1u;
      td = update_q(q, A, a, s, action, reward, ns, nt, lr, gamma, alive);
      // replay(batch_size) (agent/q.py:344-354): ONE integers(0, len(M), B), element j from
      // sub-stream j, then the B updates in order
      const bool rep = alive && loglen > 0u;
      for (int j0 = 0; j0 < B; j0 += kChunk) {
        double rr[kRounds];
        uint32_t rm[kRounds];
#pragma unroll
        for (int t = 0; t < kRounds; ++t) {
          rr[t] = 0.0;
          rm[t] = 0u;
          const int j = j0 + t * kG + a;
          if (j0 + t * kG < B) {
            const cobel_u4 blk = cobel_philox(cm >> 2, (uint32_t)j, g, COBEL_STREAM_MEMORY, R.seed);
            if (rep && j < B) {
              const uint32_t idx = cobel_bounded(cobel_word(blk, cm & 3u), loglen);
              if (appended && idx + 1u == loglen) {   // this step's record: from registers
                rr[t] = reward;
                rm[t] = meta | 0x80000000u;
              } else {
                const unsigned long long* const w = (const unsigned long long*)(rlog + idx);
                const unsigned long long w0 =
                    __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long w1 =
                    __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                rr[t] = __builtin_bit_cast(double, w0);
                rm[t] = (uint32_t)w1;
              }
            }
          }
        }
#pragma unroll
        for (int t = 0; t < kRounds; ++t) {
          if (j0 + t * kG >= B) break;
#pragma unroll
          for (int k = 0; k < kG; ++k) {
            if (j0 + t * kG + k >= B) break;
            const double r_k = __shfl(rr[t], k, kG);
            const uint32_t m_k = (uint32_t)__shfl((int)rm[t], k, kG);
            const int s_k = min((int)(m_k & 0xffu), NK - 1);
            const int ns_k = min((int)((m_k >> 8) & 0xffu), NK - 1);
            const int a_k = min((int)((m_k >> 16) & 0xffu), A - 1);
            const double td_k =
                update_q(q, A, a, s_k, a_k, r_k, ns_k, (int)((m_k >> 24) & 1u), lr, gamma, rep);
            // update_q leaves its td in the experience it is given, and the step's logs take the
            // experience after the replay (agent/q.py:214-219): a replay of the step's own
            // experience (bit 31, set where it was forwarded) leaves ITS td in the logs
            td = (m_k >> 31) ? td_k : td;
          }
        }
      }
      if (alive) cm += 1u;
    }
    if (alive) {
      if (head && R.trace && row < R.trace_cap) {
        double* const t = R.trace + ((size_t)i * R.trace_cap + row) * COBEL_QSEQ_ROW;
        t[0] = (double)s;
        t[1] = (double)action;
        t[2] = reward;
        t[3] = (double)ns;
        t[4] = (double)nt;
        t[5] = td;
        row += 1;
      }
      l_s = s;
      l_ns = ns;
      l_nt = nt;
      l_r = reward;
      l_td = td;
      cs += 1;
      if (end) ct += 1;
      trew += reward;
      last_action = action;
      executed += 1ull;
      budget -= 1;
      if (end || cs >= R.steps_per_trial) {   // the trial is over, or cut by the cap
        const int t = R.trial_first + done;
        if (head && t >= 0 && t < R.trial_cap) {
          const size_t o = (size_t)i * R.trial_cap + t;
          if (R.trial_reward) R.trial_reward[o] = trew;
          if (R.trial_steps) R.trial_steps[o] = cs - 1;
          if (R.trial_action) R.trial_action[o] = last_action;
        }
        done += 1;
        mid = false;
      }
      alive = done < R.trials && budget > 0;
    }
  }

  for (int k = 0; k < NK; ++k)
    if (mine) R.Q[((size_t)i * NK + k) * A + a] = q[k * A + a];
  if (head) {
    S.cur_trial[i] = ct;
    S.cur_step[i] = cs;
    R.mid[i] = mid ? 1 : 0;
    R.trew[i] = trew;
    R.pol_ctr[i] = cp;
    if (learn) {
      R.mem_ctr[i] = cm;
      R.log_len[i] = (int32_t)loglen;
    }
    if (R.trace) R.trace_len[i] = row;
    if (R.last && executed) {
      double* const t = R.last + (size_t)i * COBEL_QSEQ_ROW;
      t[0] = (double)l_s;
      t[1] = (double)last_action;
      t[2] = l_r;
      t[3] = (double)l_ns;
      t[4] = (double)l_nt;
      t[5] = l_td;
    }
    if (R.steps_done && executed) atomicAdd(R.steps_done, executed);
  }
}

// The stand-alone policy: one lane group per row, the routine of the run kernel
__global__ __launch_bounds__(256) void k_softmax_n(const double* __restrict__ values,
                                                   const uint8_t* __restrict__ mask,
                                                   const double* __restrict__ u,
                                                   const double* __restrict__ beta, int beta_rows,
                                                   uint8_t* __restrict__ action_out,
                                                   double* __restrict__ probs_out, int n, int A) {
  const int lane = (int)threadIdx.x & 63;
  const int a = lane & (kG - 1);
  const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / kG;
  const bool valid = r < (long long)n;
  const size_t row = valid ? (size_t)r : 0;
  const double v = a < A ? values[row * A + a] : 0.0;
  const uint32_t allowed = mask ? (uint32_t)mask[row] : 0xffu;
  double p;
  const int action = softmax_group(v, a, A, allowed, beta[beta_rows > 1 ? row : 0], u[row], lane, p);
  if (valid) {
    if (probs_out && a < A) probs_out[row * A + a] = p;
    if (action_out && a == 0) action_out[row] = (uint8_t)action;
  }
}

int check_shape(int32_t n_keys, int32_t n_actions, const char* who) {
  COBEL_REQUIRE(n_actions >= 1 && n_actions <= COBEL_QSEQ_MAX_ACTIONS, COBEL_E_UNSUPPORTED,
                "%s: %d actions (QAgent on a Sequence serves 1 to %d)", who, n_actions,
                COBEL_QSEQ_MAX_ACTIONS);
  COBEL_REQUIRE(n_keys >= 1 && n_keys <= COBEL_QSEQ_MAX_KEYS, COBEL_E_UNSUPPORTED,
                "%s: %d distinct observations (QAgent on a Sequence serves 1 to %d)", who, n_keys,
                COBEL_QSEQ_MAX_KEYS);
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_qseq_plan(int32_t n_keys, int32_t n_actions, int32_t n, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_qseq_plan: NULL out");
  if (int rc = check_shape(n_keys, n_actions, "cobel_qseq_plan")) return rc;
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "cobel_qseq_plan: n = %d", n);
  out[0] = kG;
  out[1] = kPerWave;
  out[2] = kPerBlock;
  out[3] = (int32_t)group_blocks(n, kG);
  return COBEL_OK;
}

extern "C" int cobel_qseq_run(const cobel_seq_t* seq, const cobel_qseq_run_t* run, void* stream) {
  COBEL_REQUIRE(run, COBEL_E_ARG, "cobel_qseq_run: NULL run");
  if (int rc = check_shape(run->n_keys, run->n_actions, "cobel_qseq_run")) return rc;
  if (int rc = check_seq(seq, "cobel_qseq_run")) return rc;
  const bool learn = run->flags & COBEL_F_LEARN;
  COBEL_REQUIRE(run->Q && run->key_of_row && run->par && run->pol_ctr && run->mid && run->trew,
                COBEL_E_ARG,
                "cobel_qseq_run: Q, key_of_row, par, pol_ctr, mid and trew are required");
  COBEL_REQUIRE(!learn || (run->log && run->log_len && run->mem_ctr), COBEL_E_ARG,
                "cobel_qseq_run: training needs log, log_len and mem_ctr");
  COBEL_REQUIRE((run->log == nullptr) == (run->log_len == nullptr), COBEL_E_ARG,
                "cobel_qseq_run: log and log_len go together");
  COBEL_REQUIRE(run->n == seq->n && run->n_actions == seq->n_actions, COBEL_E_ARG,
                "cobel_qseq_run: run->n = %d, seq->n = %d; %d and %d actions", run->n, seq->n,
                run->n_actions, seq->n_actions);
  COBEL_REQUIRE(run->policy == COBEL_QSEQ_POLICY_SOFTMAX ||
                    run->policy == COBEL_QSEQ_POLICY_EPS_GREEDY,
                COBEL_E_ARG, "cobel_qseq_run: policy = %d", run->policy);
  COBEL_REQUIRE(run->par_rows == 1 || run->par_rows == run->n, COBEL_E_ARG,
                "cobel_qseq_run: par_rows = %d (1 or n = %d)", run->par_rows, run->n);
  COBEL_REQUIRE(run->steps_per_trial >= 1, COBEL_E_RANGE, "cobel_qseq_run: steps_per_trial = %d",
                run->steps_per_trial);
  COBEL_REQUIRE(run->trials >= 0 && run->trial_first >= 0 && run->trial_cap >= 0 &&
                    run->step_budget >= 0 && run->batch_size >= 0 && run->log_cap >= 0,
                COBEL_E_RANGE,
                "cobel_qseq_run: trials = %d, trial_first = %d, trial_cap = %d, batch_size = %d, "
                "log_cap = %d", run->trials, run->trial_first, run->trial_cap, run->batch_size,
                run->log_cap);
  COBEL_REQUIRE((run->trace == nullptr) == (run->trace_len == nullptr) &&
                    (!run->trace || run->trace_cap >= 0),
                COBEL_E_ARG, "cobel_qseq_run: trace and trace_len go together");
  COBEL_REQUIRE((((uintptr_t)run->Q | (uintptr_t)run->par | (uintptr_t)run->log |
                  (uintptr_t)run->trew | (uintptr_t)run->trial_reward | (uintptr_t)run->trace |
                  (uintptr_t)run->last | (uintptr_t)run->steps_done) & 7u) == 0 &&
                    (((uintptr_t)run->key_of_row | (uintptr_t)run->pol_ctr |
                      (uintptr_t)run->mem_ctr | (uintptr_t)run->log_len |
                      (uintptr_t)run->instance_ids | (uintptr_t)run->mid |
                      (uintptr_t)run->trial_steps | (uintptr_t)run->trial_action |
                      (uintptr_t)run->trace_len) & 3u) == 0,
                COBEL_E_ARG, "cobel_qseq_run: misaligned argument");
  if (seq->n == 0 || run->trials == 0) return COBEL_OK;
  qseq_args K;
  K.s = *seq;
  K.r = *run;
  K.stride = q_stride(run->n_keys, run->n_actions);
  const size_t lds = (size_t)kPerBlock * K.stride * sizeof(double);
  COBEL_HIP_TRY(cobel_launch(k_qseq_run, dim3(group_blocks(seq->n, kG)), dim3(64 * kWaves), lds,
                             (hipStream_t)stream, K));
  return COBEL_OK;
}

extern "C" int cobel_softmax_n(const double* values, const uint8_t* mask, const double* u,
                               const double* beta, int32_t beta_rows, uint8_t* action_out,
                               double* probs_out, int32_t n, int32_t n_actions, void* stream) {
  COBEL_REQUIRE(n_actions >= 1 && n_actions <= COBEL_QSEQ_MAX_ACTIONS, COBEL_E_UNSUPPORTED,
                "cobel_softmax_n: %d actions (1 to %d)", n_actions, COBEL_QSEQ_MAX_ACTIONS);
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "cobel_softmax_n: n = %d", n);
  if (n == 0) return COBEL_OK;
  COBEL_REQUIRE(values && u && beta, COBEL_E_ARG, "cobel_softmax_n: NULL argument");
  COBEL_REQUIRE(beta_rows == 1 || beta_rows == n, COBEL_E_ARG,
                "cobel_softmax_n: beta_rows = %d (1 or n = %d)", beta_rows, n);
  COBEL_REQUIRE((((uintptr_t)values | (uintptr_t)u | (uintptr_t)beta | (uintptr_t)probs_out) &
                 7u) == 0,
                COBEL_E_ARG, "cobel_softmax_n: misaligned argument");
  const long long lanes = (long long)n * kG;
  hipLaunchKernelGGL(k_softmax_n, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, values, mask, u, beta, beta_rows, action_out, probs_out,
                     n, n_actions);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
