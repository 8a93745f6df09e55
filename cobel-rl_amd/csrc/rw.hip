// Rescorla-Wagner agents on a Sequence environment (agent/rw.py, interface/sequence.py and
// policy/scalar.py of the reference): the trial loops of a whole session in one launch, the weights,
// the instance's position in its schedule and its draw counter in registers, the schedule tables
// read in place (they are shared by all instances and small: they stay in L2).
//
// Packing.  An instance has D weights (D <= 64).  It takes a group of G lanes, G = D rounded up to
// a power of two, one lane per weight; a wavefront holds 64 / G instances, a workgroup four
// wavefronts.  Lanes beyond D, and the groups of a last wavefront that n does not fill, carry zeros
// and store nothing.
//
// Summation order of W @ state (group_sum): the products W[j] * state[j], each rounded, are the
// leaves of a balanced binary tree over G leaves, leaves D .. G - 1 being +0.0; adjacent leaves are
// added first: ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)) ...  Every lane of the group ends
// with the same bits (IEEE addition commutes), so value, policy and draw are evaluated by all lanes
// of a group alike and nothing is broadcast.  With at most two non-zero products any order gives the
// same sum (up to the sign of a zero); the reference's BLAS may fuse multiply and add, so it agrees
// in the last bit only where the products are exact (one-hot and power-of-two stimuli).
//
// Instances of one wavefront may follow schedules of different trial lengths and Threshold draws
// only inside its window, so the groups drift apart: the loop runs while any lane is alive, the
// shuffles stay in wave-uniform control flow, and everything an instance does is predicated on its
// own `alive`.  Table indices are clamped before use: a lane that is not alive still loads, from
// element 0.
//
// The file is compiled with -ffp-contract=off: lr * (v - target) * state is two rounded
// multiplications, the subtraction from W a third rounding, as NumPy evaluates it.
#include "cobel_seq.h"

namespace {

using namespace cobel_seq;

// int(action) of interface/sequence.py:155 for a float64 (truncation; what Python refuses — NaN,
// infinities — and what does not fit becomes a bound)
__device__ __forceinline__ int trunc_int(double v) {
  if (!(v == v)) return 0;
  if (v >= 2147483647.0) return 2147483647;
  if (v <= -2147483648.0) return (-2147483647 - 1);
  return (int)v;
}

struct rw_args {
  cobel_seq_t s;
  cobel_rw_run_t r;
  int G;
};

__global__ __launch_bounds__(64 * kWaves) void k_rw_run(const rw_args K) {
  const cobel_seq_t& S = K.s;
  const cobel_rw_run_t& R = K.r;
  const int G = K.G, D = S.dim;
  const int per_wave = 64 / G;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int j = lane & (G - 1);
  const long long inst = ((long long)blockIdx.x * kWaves + wave) * per_wave + lane / G;
  const bool valid = inst < (long long)S.n;
  const int i = valid ? (int)inst : 0;
  const bool mine = valid && j < D;      // this lane holds a weight
  const bool head = valid && j == 0;     // ... and writes what the instance has one of
  const bool learn = R.flags & COBEL_F_LEARN;
  const uint32_t g = R.instance_ids ? R.instance_ids[i] : R.instance_base + (uint32_t)i;
  const int jc = j < D ? j : 0;

  double w = mine ? R.W[(size_t)i * D + j] : 0.0;
  const double lr = R.lr[(size_t)(R.lr_rows > 1 ? i : 0) * D + jc];
  const double* const pp = R.pol ? R.pol + (size_t)(R.pol_rows > 1 ? i : 0) * 4 : nullptr;
  const double p_thr = pp ? pp[0] : 0.0, p_win = pp ? pp[1] : 0.0, p_scale = pp ? pp[2] : 0.0,
               p_vmax = pp ? pp[3] : 1.0;
  const int32_t* const toff = trial_offsets(S, i);

  int ct = S.cur_trial[i], cs = S.cur_step[i];
  bool mid = R.mid[i] != 0;
  double trew = R.trew[i];
  uint32_t cp = R.pol_ctr ? R.pol_ctr[i] : 0u;
  int done = 0, last_action = 0;
  long long budget = R.step_budget > 0 ? (long long)R.step_budget : 0x7fffffffffffffffll;
  unsigned long long executed = 0;
  int row = (R.trace && valid) ? R.trace_len[i] : 0;
  bool alive = valid && R.trials > 0;

  while (__ballot(alive) != 0ull) {
    if (alive && !mid) {   // Sequence.reset (interface/sequence.py:188-204)
      cs = 0;
      trew = 0.0;
      mid = true;
    }
    int base, len;
    const int at = step_at(S, toff, ct, cs, base, len);
    const int oi = clampi(S.step_obs[at], 0, S.n_obs - 1);
    const double x = (mine && alive) ? S.obs_table[(size_t)oi * D + j] : 0.0;
    // predict_on_batch (agent/rw.py:176-192)
    const double v = group_sum(w * x, G);
    // select_action (policy/scalar.py)
    int action;
    if (R.policy == COBEL_RW_POLICY_NONE) {
      action = trunc_int(v);
    } else if (R.policy == COBEL_RW_POLICY_THRESHOLD) {
      const double vn = v / p_vmax;
      action = abs(R.code_reverse - (vn > p_thr ? 1 : 0));
      if (vn > p_thr - p_win && vn < p_thr + p_win) {
        if (alive) {
          action = (int)cobel_draw_bounded(cp, 0u, g, R.pol_stream, R.seed, 2u);
          cp += 1u;
        }
      }
    } else {
      double prob = v / p_vmax;
      if (R.policy == COBEL_RW_POLICY_SIGMOID)
        prob = 1.0 / (1.0 + exp(-(prob - p_thr) * p_scale));
      const double u = cobel_draw_u01(cp, 0u, g, R.pol_stream, R.seed);
      if (alive) cp += 1u;
      action = abs(R.code_reverse - (u < prob ? 1 : 0));
    }
    // Sequence.step (interface/sequence.py:129-186)
    const double reward = step_reward(S, at, action);
    const bool end = cs + 1 >= len;
    if (alive) {
      if (learn) {   // W -= learning_rate * (v - target) * state (agent/rw.py:110, 303-309)
        double target = reward;
        if (R.policy != COBEL_RW_POLICY_NONE)
          target = ((action == 0 && reward > 0.0) || (action == 1 && reward < 0.0)) ? 1.0 : 0.0;
        const double t1 = lr * (v - target);
        const double t2 = t1 * x;
        w = w - t2;
      }
      if (head && R.trace && row < R.trace_cap) {
        double* const t = R.trace + ((size_t)i * R.trace_cap + row) * 4;
        t[0] = v;
        // (RescorlaWagner: int(value) as Python has it, beyond 32 bits too)
        t[1] = R.policy == COBEL_RW_POLICY_NONE ? trunc(v) : (double)action;
        t[2] = reward;
        t[3] = end ? 1.0 : 0.0;
        row += 1;
      }
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

  if (mine) R.W[(size_t)i * D + j] = w;
  if (head) {
    S.cur_trial[i] = ct;
    S.cur_step[i] = cs;
    R.mid[i] = mid ? 1 : 0;
    R.trew[i] = trew;
    if (R.pol_ctr) R.pol_ctr[i] = cp;
    if (R.trace) R.trace_len[i] = row;
    if (R.steps_done && executed) atomicAdd(R.steps_done, executed);
  }
}

// predict_on_batch: one lane group per (instance, batch row), the same dot routine
__global__ __launch_bounds__(64 * kWaves) void k_rw_predict(const double* __restrict__ W, int n,
                                                            int D, int G,
                                                            const double* __restrict__ batch, int B,
                                                            double* __restrict__ out) {
  const int per_wave = 64 / G;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int j = lane & (G - 1);
  const long long pair = ((long long)blockIdx.x * kWaves + wave) * per_wave + lane / G;
  const bool valid = pair < (long long)n * B;
  const int i = valid ? (int)(pair / B) : 0, b = valid ? (int)(pair % B) : 0;
  const bool mine = valid && j < D;
  const double w = mine ? W[(size_t)i * D + j] : 0.0;
  const double x = mine ? batch[(size_t)b * D + j] : 0.0;
  const double v = group_sum(w * x, G);
  if (valid && j == 0) out[(size_t)i * B + b] = v;
}

// Sequence.step / Sequence.reset outside an agent's session: one lane per instance
__global__ __launch_bounds__(256) void k_seq_step(const cobel_seq_t S,
                                                  const int32_t* __restrict__ action,
                                                  double* __restrict__ obs,
                                                  double* __restrict__ reward_out,
                                                  uint8_t* __restrict__ end_out,
                                                  int32_t* __restrict__ info) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= S.n) return;
  const int D = S.dim;
  const int32_t* const toff = trial_offsets(S, i);
  const int ct = S.cur_trial[i];
  int cs = S.cur_step[i];
  int base, len;
  const int at = step_at(S, toff, ct, cs, base, len);
  if (action) {
    const int forced = S.step_action[at];
    const int a_agent = action[i];
    const double reward = step_reward(S, at, a_agent);
    cs += 1;
    const bool end = cs >= len;
    // the next step's observation, or the zero observation (row 0) at the trial's end
    const int nx = clampi(base + clampi(cs, 0, len - 1), 0, S.n_steps - 1);
    const int oi = end ? 0 : clampi(S.step_obs[nx], 0, S.n_obs - 1);
    for (int d = 0; d < D; ++d) obs[(size_t)i * D + d] = S.obs_table[(size_t)oi * D + d];
    reward_out[i] = reward;
    end_out[i] = end ? 1 : 0;
    info[2 * (size_t)i] = a_agent;
    info[2 * (size_t)i + 1] = forced;
    S.cur_step[i] = cs;
    if (end) S.cur_trial[i] = ct + 1;
  } else {
    const int oi = clampi(S.step_obs[clampi(base, 0, S.n_steps - 1)], 0, S.n_obs - 1);
    for (int d = 0; d < D; ++d) obs[(size_t)i * D + d] = S.obs_table[(size_t)oi * D + d];
    S.cur_step[i] = 0;
  }
}

}  // namespace

extern "C" int cobel_rw_plan(int32_t dim, int32_t n, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_rw_plan: NULL out");
  COBEL_REQUIRE(dim >= 1 && dim <= COBEL_RW_MAX_DIM, COBEL_E_UNSUPPORTED,
                "cobel_rw_plan: observations of %d components (the Rescorla-Wagner agents serve 1 "
                "to %d)", dim, COBEL_RW_MAX_DIM);
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "cobel_rw_plan: n = %d", n);
  const int G = group_lanes(dim);
  out[0] = G;
  out[1] = 64 / G;
  out[2] = kWaves * (64 / G);
  out[3] = (int32_t)group_blocks(n, G);
  return COBEL_OK;
}

extern "C" int cobel_rw_run(const cobel_seq_t* seq, const cobel_rw_run_t* run, void* stream) {
  if (int rc = check_seq(seq, "cobel_rw_run")) return rc;
  COBEL_REQUIRE(run && run->W && run->lr && run->mid && run->trew, COBEL_E_ARG,
                "cobel_rw_run: run, W, lr, mid and trew are required");
  COBEL_REQUIRE(run->n == seq->n, COBEL_E_ARG, "cobel_rw_run: run->n = %d, seq->n = %d", run->n,
                seq->n);
  COBEL_REQUIRE(run->policy >= COBEL_RW_POLICY_NONE && run->policy <= COBEL_RW_POLICY_SIGMOID,
                COBEL_E_ARG, "cobel_rw_run: policy = %d", run->policy);
  COBEL_REQUIRE(run->policy == COBEL_RW_POLICY_NONE || (run->pol && run->pol_ctr), COBEL_E_ARG,
                "cobel_rw_run: a policy needs its parameters (pol) and draw counters (pol_ctr)");
  COBEL_REQUIRE(run->code_reverse == 0 || run->code_reverse == 1, COBEL_E_ARG,
                "cobel_rw_run: code_reverse = %d", run->code_reverse);
  COBEL_REQUIRE((run->lr_rows == 1 || run->lr_rows == run->n) &&
                    (!run->pol || run->pol_rows == 1 || run->pol_rows == run->n),
                COBEL_E_ARG, "cobel_rw_run: lr_rows = %d, pol_rows = %d (1 or n = %d)",
                run->lr_rows, run->pol_rows, run->n);
  COBEL_REQUIRE(run->steps_per_trial >= 1, COBEL_E_RANGE, "cobel_rw_run: steps_per_trial = %d",
                run->steps_per_trial);
  COBEL_REQUIRE(run->trials >= 0 && run->trial_first >= 0 && run->trial_cap >= 0 &&
                    run->step_budget >= 0,
                COBEL_E_RANGE, "cobel_rw_run: trials = %d, trial_first = %d, trial_cap = %d",
                run->trials, run->trial_first, run->trial_cap);
  COBEL_REQUIRE((run->trace == nullptr) == (run->trace_len == nullptr) &&
                    (!run->trace || run->trace_cap >= 0),
                COBEL_E_ARG, "cobel_rw_run: trace and trace_len go together");
  COBEL_REQUIRE((((uintptr_t)run->W | (uintptr_t)run->lr | (uintptr_t)run->pol |
                  (uintptr_t)run->trew | (uintptr_t)run->trial_reward | (uintptr_t)run->trace |
                  (uintptr_t)run->steps_done) & 7u) == 0,
                COBEL_E_ARG, "cobel_rw_run: misaligned argument");
  if (seq->n == 0 || run->trials == 0) return COBEL_OK;
  rw_args K;
  K.s = *seq;
  K.r = *run;
  K.G = group_lanes(seq->dim);
  COBEL_HIP_TRY(cobel_launch(k_rw_run, dim3(group_blocks(seq->n, K.G)), dim3(64 * kWaves), 0,
                             (hipStream_t)stream, K));
  return COBEL_OK;
}

extern "C" int cobel_rw_predict(const double* W, int32_t n, int32_t dim, const double* batch,
                                int32_t n_batch, double* out, void* stream) {
  COBEL_REQUIRE(dim >= 1 && dim <= COBEL_RW_MAX_DIM, COBEL_E_UNSUPPORTED,
                "cobel_rw_predict: observations of %d components (the Rescorla-Wagner agents serve "
                "1 to %d)", dim, COBEL_RW_MAX_DIM);
  COBEL_REQUIRE(n >= 0 && n_batch >= 0, COBEL_E_RANGE, "cobel_rw_predict: n = %d, batch of %d", n,
                n_batch);
  if (n == 0 || n_batch == 0) return COBEL_OK;
  COBEL_REQUIRE(W && batch && out, COBEL_E_ARG, "cobel_rw_predict: NULL argument");
  COBEL_REQUIRE((((uintptr_t)W | (uintptr_t)batch | (uintptr_t)out) & 7u) == 0, COBEL_E_ARG,
                "cobel_rw_predict: misaligned argument");
  COBEL_REQUIRE((long long)n * n_batch <= 0x7fffffffll, COBEL_E_RANGE,
                "cobel_rw_predict: %d instances x %d rows", n, n_batch);
  const int G = group_lanes(dim);
  hipLaunchKernelGGL(k_rw_predict, dim3(group_blocks((long long)n * n_batch, G)), dim3(64 * kWaves),
                     0, (hipStream_t)stream, W, n, dim, G, batch, n_batch, out);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_seq_step(const cobel_seq_t* seq, const int32_t* action, double* obs,
                              double* reward, uint8_t* end, int32_t* info, void* stream) {
  if (int rc = check_seq(seq, "cobel_seq_step")) return rc;
  if (seq->n == 0) return COBEL_OK;
  COBEL_REQUIRE(action && obs && reward && end && info, COBEL_E_ARG,
                "cobel_seq_step: NULL argument");
  COBEL_REQUIRE((((uintptr_t)obs | (uintptr_t)reward) & 7u) == 0 &&
                    (((uintptr_t)action | (uintptr_t)info) & 3u) == 0,
                COBEL_E_ARG, "cobel_seq_step: misaligned argument");
  hipLaunchKernelGGL(k_seq_step, dim3((unsigned)((seq->n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, *seq, action, obs, reward, end, info);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_seq_reset(const cobel_seq_t* seq, double* obs, void* stream) {
  if (int rc = check_seq(seq, "cobel_seq_reset")) return rc;
  if (seq->n == 0) return COBEL_OK;
  COBEL_REQUIRE(obs && ((uintptr_t)obs & 7u) == 0, COBEL_E_ARG,
                "cobel_seq_reset: obs must be given, aligned");
  hipLaunchKernelGGL(k_seq_step, dim3((unsigned)((seq->n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, *seq, (const int32_t*)nullptr, obs, (double*)nullptr,
                     (uint8_t*)nullptr, (int32_t*)nullptr);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
