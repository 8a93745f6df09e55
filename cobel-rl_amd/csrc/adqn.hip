// ADQN (agent/adqn.py of the reference) on a Sequence environment: the memory that keeps every
// experience (memory/adqn.py) and everything of one lockstep training step that is not the network.
//
// One wavefront serves one instance, four wavefronts a workgroup; a wavefront whose instance does
// not exist, or has no trial of the session left, leaves at once (nothing here meets at a barrier).
// The memory of instance j is rows [j][0 .. count[j]) of caller-owned arrays of capacity cap.
//
// store (memory/adqn.py:119-138): lane e & 63 owns entry e for good — it multiplies its priority by
// decay at every later store and it wrote it in the first place — so the k stores of one launch
// need no ordering between lanes.  The state row is copied by the lanes below dim.
//
// sample (memory/adqn.py:156-164): the count entries are cut into 64 consecutive chunks of
// c = ceil(count / 64); lane l sums its chunk left to right, the lanes' sums meet in the balanced
// tree of cobel_seq::group_sum (prob_sum) and, for the probabilities, in a Hillis-Steele inclusive
// scan whose value of lane l - 1 is what lane l starts its chunk from.  The normalised cdf goes to
// the scratch row of the instance; a workgroup-scope fence later every lane that holds a draw counts
// the entries its u has passed.  The count does not care whether the cdf is monotone at a chunk
// seam.  The file is compiled with -ffp-contract=off: every operation rounds once, and
// tests/adqn_common.py restates this order bit for bit.
//
// step: Sequence.reset / step through cobel_seq.h, store, sample, the position, the trial
// bookkeeping of k_rw_run and k_anet_run, and the observation row the network evaluates next.
#include "cobel_seq.h"
#include "cobel_rng.h"

namespace {

using namespace cobel_seq;

struct adqn_args {
  cobel_seq_t s;
  cobel_adqn_mem_t m;
  cobel_adqn_step_t r;
};

__device__ __forceinline__ uint32_t instance_of(const cobel_adqn_mem_t& M, int i) {
  return M.instance_ids ? M.instance_ids[i] : M.instance_base + (uint32_t)i;
}

// One experience appended at entry cnt < cap of instance i; src: the dim components of its state
__device__ __forceinline__ void mem_store(const cobel_adqn_mem_t& M, int i, int lane, int cnt,
                                          const double* __restrict__ src, double action,
                                          double reward) {
  const size_t base = (size_t)i * M.cap;
  double* const pr = M.priorities + base;
  for (int e = lane; e < cnt; e += 64) pr[e] = pr[e] * M.decay;
  if (lane < M.dim) M.states[(base + cnt) * M.dim + lane] = src[lane];
  if (lane == (cnt & 63)) {
    const double err = action - reward;
    M.reinforcements[base + cnt] = reward;
    M.errors[base + cnt] = err;
    pr[cnt] = (M.flags & COBEL_ADQN_RPE) ? fabs(err) : 1.0;
  }
}

// The batch of instance i from its n >= 1 entries, draw counter ctr.  To be called by all 64 lanes.
__device__ __forceinline__ void mem_sample(const cobel_adqn_mem_t& M, int i, int lane, int n,
                                           uint32_t ctr, int B, bool f64, int32_t* idx,
                                           int32_t* in_index, void* targets, int32_t* idx_copy) {
  const size_t base = (size_t)i * M.cap;
  const double* const pr = M.priorities + base;
  double* const cdf = M.scratch + base;
  const int c = (n + 63) >> 6;
  const int lo = min(lane * c, n), hi = min(lo + c, n);
  double s = 0.0;
  for (int e = lo; e < hi; ++e) s = s + pr[e];
  const double prob_sum = group_sum(s, 64);
  const bool uniform = prob_sum == 0.0;
  const double each = 1.0 / (double)n;
  double t = 0.0;
  for (int e = lo; e < hi; ++e) t = t + (uniform ? each : pr[e] / prob_sum);
  double inc = t;
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(inc, o);
    if (lane >= o) inc = inc + up;
  }
  double excl = __shfl_up(inc, 1);
  if (lane == 0) excl = 0.0;
  const double last = __shfl(excl + t, (n - 1) / c);   // the cdf at entry n - 1
  double run = 0.0;
  for (int e = lo; e < hi; ++e) {
    run = run + (uniform ? each : pr[e] / prob_sum);
    cdf[e] = (excl + run) / last;
  }
  __threadfence_block();
  const uint32_t g = instance_of(M, i);
  for (int b = lane; b < B; b += 64) {
    const double u = cobel_draw_u01(ctr, (uint32_t)b, g, COBEL_STREAM_ADQN_MEMORY, M.seed);
    int k = 0;
    for (int e = 0; e < n; ++e) k += cdf[e] <= u ? 1 : 0;
    k = k < n ? k : n - 1;
    const size_t o = (size_t)i * B + b;
    if (idx) idx[o] = k;
    if (idx_copy) idx_copy[b] = k;
    in_index[o] = (int32_t)(base + k);
    const double r = M.reinforcements[base + k];
    if (f64)
      ((double*)targets)[o] = r;
    else
      ((float*)targets)[o] = (float)r;
  }
}

__global__ __launch_bounds__(64 * kWaves) void k_adqn_store(const cobel_adqn_mem_t M, int K,
                                                            const double* __restrict__ states,
                                                            const double* __restrict__ actions,
                                                            const double* __restrict__ rewards) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const long long inst = (long long)blockIdx.x * kWaves + wave;
  if (inst >= (long long)M.n) return;
  const int i = (int)inst;
  int cnt = M.count[i];
  for (int k = 0; k < K && cnt < M.cap; ++k, ++cnt) {
    const size_t at = (size_t)i * K + k;
    mem_store(M, i, lane, cnt, states + at * M.dim, actions[at], rewards[at]);
  }
  if (lane == 0) M.count[i] = cnt;
}

__global__ __launch_bounds__(64 * kWaves) void k_adqn_sample(const cobel_adqn_mem_t M, int B,
                                                             int f64, int32_t* idx,
                                                             int32_t* in_index, void* targets) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const long long inst = (long long)blockIdx.x * kWaves + wave;
  if (inst >= (long long)M.n) return;
  const int i = (int)inst;
  const int n = min(M.count[i], M.cap);
  if (n < 1) return;
  const uint32_t ctr = M.draw_ctr[i];
  mem_sample(M, i, lane, n, ctr, B, f64 != 0, idx, in_index, targets, nullptr);
  if (lane == 0) M.draw_ctr[i] = ctr + 1u;
}

__global__ __launch_bounds__(64 * kWaves) void k_adqn_step(const adqn_args K) {
  const cobel_seq_t& S = K.s;
  const cobel_adqn_mem_t& M = K.m;
  const cobel_adqn_step_t& R = K.r;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const long long inst = (long long)blockIdx.x * kWaves + wave;
  if (inst >= (long long)S.n) return;
  const int i = (int)inst;
  const bool head = lane == 0;
  int done = R.done[i];
  if (done >= R.trials) {   // (the whole wavefront: the instance is one)
    if (head) {
      R.active[i] = 0;
      R.alive[i] = 0;
    }
    return;
  }
  const bool learn = R.flags & COBEL_F_LEARN;
  const int D = S.dim;
  const int32_t* const toff = trial_offsets(S, i);
  int ct = S.cur_trial[i], cs = S.cur_step[i];
  double trew = R.trew[i];
  if (R.mid[i] == 0) {   // Sequence.reset (interface/sequence.py:188-204)
    cs = 0;
    trew = 0.0;
  }
  int base, len;
  const int at = step_at(S, toff, ct, cs, base, len);
  const int oi = clampi(S.step_obs[at], 0, S.n_obs - 1);
  // the action is the value itself (agent/adqn.py:134)
  const double value = R.is_float64 ? ((const double*)R.value)[i]
                                    : (double)((const float*)R.value)[i];
  // Sequence.step (interface/sequence.py:129-186)
  const double reward = step_reward(S, at, 0);
  const bool end = cs + 1 >= len;
  int row = R.trace ? R.trace_len[i] : 0;
  const bool keep = R.trace && row < R.trace_cap;
  int cnt = min(M.count[i], M.cap);
  bool stored = false;
  if (learn && cnt < M.cap) {
    // memory.store (memory/adqn.py:119-138), then replay's sample_batch (agent/adqn.py:234)
    mem_store(M, i, lane, cnt, S.obs_table + (size_t)oi * D, value, reward);
    cnt += 1;
    stored = true;
    __threadfence_block();
    const uint32_t ctr = M.draw_ctr[i];
    mem_sample(M, i, lane, cnt, ctr, R.batch, R.is_float64 != 0, R.idx, R.in_index, R.targets,
               (keep && R.idx_trace) ? R.idx_trace + ((size_t)i * R.trace_cap + row) * R.batch
                                     : nullptr);
    if (head) {
      M.count[i] = cnt;
      M.draw_ctr[i] = ctr + 1u;
    }
  }
  cs += 1;
  if (end) ct += 1;
  trew = trew + reward;
  const bool over = end || cs >= R.steps_per_trial;   // the trial is over, or cut by the cap
  // what the instance sees next: the trial's next step, or the first step of the trial a reset
  // begins (a trial cut by the cap is replayed from its first step)
  int next_row = 0;
  if (!over)
    next_row = S.step_obs[clampi(at + 1, 0, S.n_steps - 1)];
  else if (ct < S.n_trials)
    next_row = S.step_obs[clampi(toff[ct], 0, S.n_steps - 1)];
  if (!head) return;
  if (keep) {
    double* const t = R.trace + ((size_t)i * R.trace_cap + row) * 3;
    t[0] = value;
    t[1] = reward;
    t[2] = end ? 1.0 : 0.0;
    R.trace_len[i] = row + 1;
  }
  if (R.step_rec) {
    double* const t = R.step_rec + (size_t)i * 4;
    t[0] = value;
    t[1] = reward;
    t[2] = end ? 1.0 : 0.0;
    t[3] = end ? 0.0 : 1.0;
  }
  if (over) {
    const int t = R.trial_first + done;
    if (t >= 0 && t < R.trial_cap) {
      const size_t o = (size_t)i * R.trial_cap + t;
      if (R.trial_reward) R.trial_reward[o] = trew;
      if (R.trial_steps) R.trial_steps[o] = cs - 1;
    }
    done += 1;
  }
  S.cur_trial[i] = ct;
  S.cur_step[i] = cs;
  R.mid[i] = over ? 0 : 1;
  R.trew[i] = trew;
  R.done[i] = done;
  R.ep_index[i] = clampi(next_row, 0, S.n_obs - 1);
  R.active[i] = stored ? 1 : 0;
  R.alive[i] = done < R.trials ? 1 : 0;
  if (R.steps_done) atomicAdd(R.steps_done, 1ull);
}

unsigned blocks_of(int n) { return (unsigned)((n + kWaves - 1) / kWaves); }

int check_mem(const cobel_adqn_mem_t* m, bool draws, const char* who) {
  COBEL_REQUIRE(m, COBEL_E_ARG, "%s: NULL memory", who);
  COBEL_REQUIRE(m->dim >= 1 && m->dim <= COBEL_RW_MAX_DIM, COBEL_E_UNSUPPORTED,
                "%s: observations of %d components (the ADQN memory serves 1 to %d)", who, m->dim,
                COBEL_RW_MAX_DIM);
  COBEL_REQUIRE(m->n >= 0, COBEL_E_RANGE, "%s: n = %d", who, m->n);
  COBEL_REQUIRE(m->cap >= 0 && (long long)m->n * m->cap < 0x80000000ll, COBEL_E_RANGE,
                "%s: %d instances of capacity %d (n cap must stay below 2^31)", who, m->n, m->cap);
  COBEL_REQUIRE(m->decay >= 0.0 && m->decay <= 1.0, COBEL_E_ARG, "%s: decay = %g (0 to 1)", who,
                m->decay);
  COBEL_REQUIRE(m->count_min >= 0 && m->count_min <= m->count_max && m->count_max <= m->cap,
                COBEL_E_RANGE, "%s: counts of %d to %d in a capacity of %d", who, m->count_min,
                m->count_max, m->cap);
  COBEL_REQUIRE(m->states && m->reinforcements && m->errors && m->priorities && m->count &&
                    (!draws || (m->draw_ctr && m->scratch)),
                COBEL_E_ARG, "%s: NULL array of the memory", who);
  COBEL_REQUIRE((((uintptr_t)m->states | (uintptr_t)m->reinforcements | (uintptr_t)m->errors |
                  (uintptr_t)m->priorities | (uintptr_t)m->scratch) & 7u) == 0 &&
                    (((uintptr_t)m->count | (uintptr_t)m->draw_ctr |
                      (uintptr_t)m->instance_ids) & 3u) == 0,
                COBEL_E_ARG, "%s: misaligned array of the memory", who);
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_adqn_plan(int32_t dim, int32_t n, int32_t cap, int64_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_adqn_plan: NULL out");
  COBEL_REQUIRE(dim >= 1 && dim <= COBEL_RW_MAX_DIM, COBEL_E_UNSUPPORTED,
                "cobel_adqn_plan: observations of %d components (the ADQN memory serves 1 to %d)",
                dim, COBEL_RW_MAX_DIM);
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "cobel_adqn_plan: n = %d", n);
  COBEL_REQUIRE(cap >= 0 && (long long)n * cap < 0x80000000ll, COBEL_E_RANGE,
                "cobel_adqn_plan: %d instances of capacity %d (n cap must stay below 2^31)", n, cap);
  out[0] = kWaves;
  out[1] = blocks_of(n);
  out[2] = (int64_t)n * cap * (int64_t)sizeof(double);
  out[3] = 64;
  return COBEL_OK;
}

extern "C" int cobel_adqn_store(const cobel_adqn_mem_t* mem, int32_t k, const double* states,
                                const double* actions, const double* rewards, void* stream) {
  if (int rc = check_mem(mem, false, "cobel_adqn_store")) return rc;
  COBEL_REQUIRE(k >= 0, COBEL_E_RANGE, "cobel_adqn_store: k = %d", k);
  COBEL_REQUIRE((long long)mem->count_max + k <= mem->cap, COBEL_E_RANGE,
                "cobel_adqn_store: %d experiences on top of %d pass the capacity of %d", k,
                mem->count_max, mem->cap);
  if (mem->n == 0 || k == 0) return COBEL_OK;
  COBEL_REQUIRE(states && actions && rewards, COBEL_E_ARG, "cobel_adqn_store: NULL argument");
  COBEL_REQUIRE((((uintptr_t)states | (uintptr_t)actions | (uintptr_t)rewards) & 7u) == 0,
                COBEL_E_ARG, "cobel_adqn_store: misaligned argument");
  hipLaunchKernelGGL(k_adqn_store, dim3(blocks_of(mem->n)), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, *mem, k, states, actions, rewards);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_adqn_sample(const cobel_adqn_mem_t* mem, int32_t batch, int32_t is_float64,
                                 int32_t* idx, int32_t* in_index, void* targets, void* stream) {
  if (int rc = check_mem(mem, true, "cobel_adqn_sample")) return rc;
  COBEL_REQUIRE(batch >= 1 && (long long)mem->n * batch < 0x80000000ll, COBEL_E_RANGE,
                "cobel_adqn_sample: batch of %d for %d instances", batch, mem->n);
  if (mem->n == 0) return COBEL_OK;
  COBEL_REQUIRE(mem->count_min >= 1, COBEL_E_RANGE,
                "cobel_adqn_sample: an empty memory has nothing to draw ('a' cannot be empty)");
  COBEL_REQUIRE(in_index && targets, COBEL_E_ARG, "cobel_adqn_sample: NULL argument");
  COBEL_REQUIRE((((uintptr_t)idx | (uintptr_t)in_index) & 3u) == 0 &&
                    ((uintptr_t)targets & (is_float64 ? 7u : 3u)) == 0,
                COBEL_E_ARG, "cobel_adqn_sample: misaligned argument");
  hipLaunchKernelGGL(k_adqn_sample, dim3(blocks_of(mem->n)), dim3(64 * kWaves), 0,
                     (hipStream_t)stream, *mem, batch, is_float64, idx, in_index, targets);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_adqn_step(const cobel_seq_t* seq, const cobel_adqn_mem_t* mem,
                               const cobel_adqn_step_t* run, void* stream) {
  if (int rc = check_seq(seq, "cobel_adqn_step")) return rc;
  COBEL_REQUIRE(run, COBEL_E_ARG, "cobel_adqn_step: NULL run");
  const bool learn = run->flags & COBEL_F_LEARN;
  if (int rc = check_mem(mem, learn, "cobel_adqn_step")) return rc;
  COBEL_REQUIRE(run->n == seq->n && mem->n == seq->n && mem->dim == seq->dim, COBEL_E_ARG,
                "cobel_adqn_step: run->n = %d, mem->n = %d, seq->n = %d; mem->dim = %d, seq->dim = %d",
                run->n, mem->n, seq->n, mem->dim, seq->dim);
  COBEL_REQUIRE(run->value && run->ep_index && run->active && run->alive && run->done &&
                    run->mid && run->trew,
                COBEL_E_ARG,
                "cobel_adqn_step: value, ep_index, active, alive, done, mid and trew are required");
  COBEL_REQUIRE(!learn || (run->in_index && run->targets), COBEL_E_ARG,
                "cobel_adqn_step: in_index and targets are required to learn");
  COBEL_REQUIRE(!learn || (run->batch >= 1 && (long long)run->n * run->batch < 0x80000000ll),
                COBEL_E_RANGE, "cobel_adqn_step: batch of %d for %d instances", run->batch, run->n);
  COBEL_REQUIRE(!learn || mem->count_max + 1 <= mem->cap, COBEL_E_RANGE,
                "cobel_adqn_step: one experience on top of %d passes the capacity of %d",
                mem->count_max, mem->cap);
  COBEL_REQUIRE(run->steps_per_trial >= 1, COBEL_E_RANGE, "cobel_adqn_step: steps_per_trial = %d",
                run->steps_per_trial);
  COBEL_REQUIRE(run->trials >= 0 && run->trial_first >= 0 && run->trial_cap >= 0, COBEL_E_RANGE,
                "cobel_adqn_step: trials = %d, trial_first = %d, trial_cap = %d", run->trials,
                run->trial_first, run->trial_cap);
  COBEL_REQUIRE((run->trace == nullptr) == (run->trace_len == nullptr) &&
                    (!run->trace || run->trace_cap >= 0) && (!run->idx_trace || run->trace),
                COBEL_E_ARG, "cobel_adqn_step: trace and trace_len go together, idx_trace with them");
  COBEL_REQUIRE((((uintptr_t)run->trew | (uintptr_t)run->trial_reward | (uintptr_t)run->step_rec |
                  (uintptr_t)run->trace | (uintptr_t)run->steps_done) & 7u) == 0 &&
                    (((uintptr_t)run->in_index | (uintptr_t)run->idx | (uintptr_t)run->ep_index |
                      (uintptr_t)run->done | (uintptr_t)run->mid | (uintptr_t)run->trial_steps |
                      (uintptr_t)run->idx_trace | (uintptr_t)run->trace_len) & 3u) == 0 &&
                    (((uintptr_t)run->value | (uintptr_t)run->targets) &
                     (run->is_float64 ? 7u : 3u)) == 0,
                COBEL_E_ARG, "cobel_adqn_step: misaligned argument");
  if (seq->n == 0 || run->trials == 0) return COBEL_OK;
  adqn_args K;
  K.s = *seq;
  K.m = *mem;
  K.r = *run;
  COBEL_HIP_TRY(cobel_launch(k_adqn_step, dim3(blocks_of(seq->n)), dim3(64 * kWaves), 0,
                             (hipStream_t)stream, K));
  return COBEL_OK;
}
