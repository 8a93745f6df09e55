// AssociativeNetwork (agent/anet.py of the reference, Donoso et al. 2021) on a Sequence environment:
// the trial loops of a whole session in one launch, both weight matrices, the instance's position
// in its schedule and its two draw counters in registers, the schedule tables read in place.
//
// Packing is k_rw_run's (rw.hip, cobel_seq.h).  An instance has D observation components (D <= 64)
// and NA = n_actions - 1 outputs (1 <= NA <= 8).  It takes a group of G lanes, G = D rounded up to
// a power of two; lane j holds row j of the excitatory and of the inhibitory matrix, up to 2 x 8
// doubles.  A wavefront holds 64 / G instances, a workgroup four wavefronts.  Lanes beyond D, and
// the groups of a last wavefront that n does not fill, carry zeros and store nothing.  The rows are
// indexed with unrolled compares against the action, never with a runtime subscript, which would
// send them to scratch memory.  saturation and learning_rate are per-weight arrays as well; they
// are read from memory, one value each per step, when an update needs them.
//
// Per step (anet.py:311-333): for every output a the two dot products state @ We[:, a] and
// state @ Wi[:, a] in the order of group_sum — rounded products as the leaves of a balanced tree over
// G leaves, adjacent leaves first — then q[a] = (e - i) + noise * u[a], u[a] being the double draw
// agent_ctr + a of COBEL_STREAM_AGENT (rng.random(NA) takes them in column order); the counter
// advances by NA.  The selection is EpsilonGreedy's over the NA values in float64 with exact ties,
// one double draw of the policy's stream, also where NA = 1.  update_q (:335-356) changes column
// `action` of one matrix — excitatory if reward > 0, else inhibitory — in the rows whose state
// component is not zero: alpha * (sat - w) is rounded, its product with lr is rounded, the sum is
// rounded (the file is compiled with -ffp-contract=off); under linear_update the increment is
// lr * 1.0.
//
// Groups of one wavefront drift apart when their schedules differ: the loop runs while any lane is
// alive, the shuffles stay in wave-uniform control flow, and everything an instance does is
// predicated on its own `alive`.
#include "cobel_seq.h"
#include "cobel_policy.h"

namespace {

using namespace cobel_seq;

constexpr int kOut = COBEL_ANET_MAX_ACTIONS - 1;   // outputs at most

struct anet_args {
  cobel_seq_t s;
  cobel_anet_run_t r;
  int G;
};

// q of anet.py:329-333 for the rows we / wi of this lane and its state component x, the noise drawn
// at agent counter `ca`.  Every lane of the group returns the same bits.
__device__ __forceinline__ void retrieve_q(const double (&we)[kOut], const double (&wi)[kOut],
                                           double x, int NA, int G, double noise, uint32_t ca,
                                           uint32_t g, uint64_t seed, double (&q)[kOut]) {
#pragma unroll
  for (int a = 0; a < kOut; ++a) {
    q[a] = 0.0;
    if (a < NA) {   // (NA is the launch's: wave-uniform)
      const double e = group_sum(we[a] * x, G);
      const double h = group_sum(wi[a] * x, G);
      const double u = cobel_draw_u01(ca + (uint32_t)a, 0u, g, COBEL_STREAM_AGENT, seed);
      const double nz = noise * u;
      q[a] = (e - h) + nz;
    }
  }
}

// W[weight][:, action] += (lr * delta) * (state != 0) for this lane's row (anet.py:344-356)
__device__ __forceinline__ double updated(double w, double sat, double lr, double alpha,
                                          bool linear) {
  const double delta = linear ? 1.0 : alpha * (sat - w);
  const double inc = lr * delta;
  return w + inc;
}

__global__ __launch_bounds__(64 * kWaves) void k_anet_run(const anet_args K) {
  const cobel_seq_t& S = K.s;
  const cobel_anet_run_t& R = K.r;
  const int G = K.G, D = S.dim, NA = R.n_actions - 1;
  const int per_wave = 64 / G;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int j = lane & (G - 1);
  const long long inst = ((long long)blockIdx.x * kWaves + wave) * per_wave + lane / G;
  const bool valid = inst < (long long)S.n;
  const int i = valid ? (int)inst : 0;
  const bool mine = valid && j < D;      // this lane holds a row
  const bool head = valid && j == 0;     // ... and writes what the instance has one of
  const bool learn = R.flags & COBEL_F_LEARN;
  const bool linear = R.linear_update != 0;
  const uint32_t g = R.instance_ids ? R.instance_ids[i] : R.instance_base + (uint32_t)i;
  const int jc = j < D ? j : 0;
  const int width = 3 + NA;              // of a trace row

  double we[kOut], wi[kOut];
  const size_t wrow = ((size_t)i * D + jc) * NA;
#pragma unroll
  for (int a = 0; a < kOut; ++a) {
    we[a] = (mine && a < NA) ? R.We[wrow + a] : 0.0;
    wi[a] = (mine && a < NA) ? R.Wi[wrow + a] : 0.0;
  }
  const size_t srow = ((size_t)(R.sat_rows > 1 ? i : 0) * D + jc) * NA;
  const size_t lrow = ((size_t)(R.lr_rows > 1 ? i : 0) * D + jc) * NA;
  const double eps = R.eps[R.eps_rows > 1 ? i : 0];
  const int32_t* const toff = trial_offsets(S, i);

  int ct = S.cur_trial[i], cs = S.cur_step[i];
  bool mid = R.mid[i] != 0;
  double trew = R.trew[i];
  uint32_t cp = R.pol_ctr[i], ca = R.agent_ctr[i];
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
    // retrieve_q (agent/anet.py:311-333)
    double q[kOut];
    retrieve_q(we, wi, x, NA, G, R.noise, ca, g, R.seed, q);
    // select_action (policy/greedy.py:40-88)
    const double u = cobel_draw_u01(cp, 0u, g, R.pol_stream, R.seed);
    const int action = cobel_eps_greedy_select_n<double, kOut>(q, NA, 0xffu, u, eps, nullptr);
    // Sequence.step (interface/sequence.py:129-186)
    const double reward = step_reward(S, at, action);
    const bool end = cs + 1 >= len;
    // update_q (agent/anet.py:335-356): what it would read, from an element that exists
    const bool exc = reward > 0.0;
    const double sat = (exc ? R.sat_e : R.sat_i)[srow + action];
    const double lr = (exc ? R.lr_e : R.lr_i)[lrow + action];
    if (alive) {
      cp += 1u;
      ca += (uint32_t)NA;
      if (learn && x != 0.0) {
#pragma unroll
        for (int a = 0; a < kOut; ++a) {
          if (a == action) {
            if (exc)
              we[a] = updated(we[a], sat, lr, R.alpha, linear);
            else
              wi[a] = updated(wi[a], sat, lr, R.alpha, linear);
          }
        }
      }
      if (head && R.trace && row < R.trace_cap) {
        double* const t = R.trace + ((size_t)i * R.trace_cap + row) * width;
        t[0] = (double)action;
        t[1] = reward;
        t[2] = end ? 1.0 : 0.0;
#pragma unroll
        for (int a = 0; a < kOut; ++a)
          if (a < NA) t[3 + a] = q[a];
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

  if (mine) {
#pragma unroll
    for (int a = 0; a < kOut; ++a) {
      if (a < NA) {
        R.We[wrow + a] = we[a];
        R.Wi[wrow + a] = wi[a];
      }
    }
  }
  if (head) {
    S.cur_trial[i] = ct;
    S.cur_step[i] = cs;
    R.mid[i] = mid ? 1 : 0;
    R.trew[i] = trew;
    R.pol_ctr[i] = cp;
    R.agent_ctr[i] = ca;
    if (R.trace) R.trace_len[i] = row;
    if (R.steps_done && executed) atomicAdd(R.steps_done, executed);
  }
}

// retrieve_q / predict_on_batch: one lane group per (instance, batch row), the same routine
__global__ __launch_bounds__(64 * kWaves) void k_anet_predict(const cobel_anet_run_t R, int D, int G,
                                                              const double* __restrict__ batch,
                                                              int B, double* __restrict__ out) {
  const int NA = R.n_actions - 1;
  const int per_wave = 64 / G;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int j = lane & (G - 1);
  const long long pair = ((long long)blockIdx.x * kWaves + wave) * per_wave + lane / G;
  const bool valid = pair < (long long)R.n * B;
  const int i = valid ? (int)(pair / B) : 0, b = valid ? (int)(pair % B) : 0;
  const bool mine = valid && j < D;
  const int jc = j < D ? j : 0;
  const uint32_t g = R.instance_ids ? R.instance_ids[i] : R.instance_base + (uint32_t)i;
  double we[kOut], wi[kOut];
  const size_t wrow = ((size_t)i * D + jc) * NA;
#pragma unroll
  for (int a = 0; a < kOut; ++a) {
    we[a] = (mine && a < NA) ? R.We[wrow + a] : 0.0;
    wi[a] = (mine && a < NA) ? R.Wi[wrow + a] : 0.0;
  }
  const double x = mine ? batch[(size_t)b * D + j] : 0.0;
  double q[kOut];
  retrieve_q(we, wi, x, NA, G, R.noise, R.agent_ctr[i] + (uint32_t)(b * NA), g, R.seed, q);
  if (valid && j == 0) {
    double* const o = out + ((size_t)i * B + b) * NA;
#pragma unroll
    for (int a = 0; a < kOut; ++a)
      if (a < NA) o[a] = q[a];
  }
}

// (a launch of its own: every row of k_anet_predict reads the counter it was launched with)
__global__ __launch_bounds__(256) void k_anet_advance(uint32_t* __restrict__ ctr, int n,
                                                      uint32_t by) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) ctr[i] += by;
}

// update_q with one experience per instance: one lane per (instance, row)
__global__ __launch_bounds__(256) void k_anet_update(const cobel_anet_run_t R, int D,
                                                     const double* __restrict__ state,
                                                     const int32_t* __restrict__ action,
                                                     const double* __restrict__ reward) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)R.n * D) return;
  const int NA = R.n_actions - 1;
  const int i = (int)(e / D), j = (int)(e % D);
  const int a = action[i];
  if (a < 0 || a >= NA || state[e] == 0.0) return;
  const bool exc = reward[i] > 0.0;
  const size_t srow = ((size_t)(R.sat_rows > 1 ? i : 0) * D + j) * NA;
  const size_t lrow = ((size_t)(R.lr_rows > 1 ? i : 0) * D + j) * NA;
  double* const w = (exc ? R.We : R.Wi) + ((size_t)i * D + j) * NA + a;
  *w = updated(*w, (exc ? R.sat_e : R.sat_i)[srow + a], (exc ? R.lr_e : R.lr_i)[lrow + a], R.alpha,
               R.linear_update != 0);
}

int check_shape(int32_t dim, int32_t n_actions, int32_t n, const char* who) {
  COBEL_REQUIRE(dim >= 1 && dim <= COBEL_RW_MAX_DIM, COBEL_E_UNSUPPORTED,
                "%s: observations of %d components (the AssociativeNetwork serves 1 to %d)", who,
                dim, COBEL_RW_MAX_DIM);
  COBEL_REQUIRE(n_actions >= 2 && n_actions <= COBEL_ANET_MAX_ACTIONS, COBEL_E_UNSUPPORTED,
                "%s: %d actions (the AssociativeNetwork serves 2 to %d)", who, n_actions,
                COBEL_ANET_MAX_ACTIONS);
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "%s: n = %d", who, n);
  return COBEL_OK;
}

int check_weights(const cobel_anet_run_t* run, const char* who) {
  COBEL_REQUIRE(run && run->We && run->Wi, COBEL_E_ARG, "%s: run, We and Wi are required", who);
  COBEL_REQUIRE((((uintptr_t)run->We | (uintptr_t)run->Wi) & 7u) == 0, COBEL_E_ARG,
                "%s: misaligned weights", who);
  return COBEL_OK;
}

int check_rates(const cobel_anet_run_t* run, const char* who) {
  COBEL_REQUIRE(run->sat_e && run->sat_i && run->lr_e && run->lr_i, COBEL_E_ARG,
                "%s: sat_e, sat_i, lr_e and lr_i are required", who);
  COBEL_REQUIRE((run->sat_rows == 1 || run->sat_rows == run->n) &&
                    (run->lr_rows == 1 || run->lr_rows == run->n),
                COBEL_E_ARG, "%s: sat_rows = %d, lr_rows = %d (1 or n = %d)", who, run->sat_rows,
                run->lr_rows, run->n);
  COBEL_REQUIRE((((uintptr_t)run->sat_e | (uintptr_t)run->sat_i | (uintptr_t)run->lr_e |
                  (uintptr_t)run->lr_i) & 7u) == 0,
                COBEL_E_ARG, "%s: misaligned saturation or learning rate", who);
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_anet_plan(int32_t dim, int32_t n_actions, int32_t n, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_anet_plan: NULL out");
  if (int rc = check_shape(dim, n_actions, n, "cobel_anet_plan")) return rc;
  const int G = group_lanes(dim);
  out[0] = G;
  out[1] = 64 / G;
  out[2] = kWaves * (64 / G);
  out[3] = (int32_t)group_blocks(n, G);
  return COBEL_OK;
}

extern "C" int cobel_anet_run(const cobel_seq_t* seq, const cobel_anet_run_t* run, void* stream) {
  if (int rc = check_seq(seq, "cobel_anet_run")) return rc;
  if (int rc = check_weights(run, "cobel_anet_run")) return rc;
  COBEL_REQUIRE(run->n == seq->n, COBEL_E_ARG, "cobel_anet_run: run->n = %d, seq->n = %d", run->n,
                seq->n);
  if (int rc = check_shape(seq->dim, run->n_actions, run->n, "cobel_anet_run")) return rc;
  if (int rc = check_rates(run, "cobel_anet_run")) return rc;
  COBEL_REQUIRE(run->eps && run->pol_ctr && run->agent_ctr && run->mid && run->trew, COBEL_E_ARG,
                "cobel_anet_run: eps, pol_ctr, agent_ctr, mid and trew are required");
  COBEL_REQUIRE(run->eps_rows == 1 || run->eps_rows == run->n, COBEL_E_ARG,
                "cobel_anet_run: eps_rows = %d (1 or n = %d)", run->eps_rows, run->n);
  COBEL_REQUIRE(run->steps_per_trial >= 1, COBEL_E_RANGE, "cobel_anet_run: steps_per_trial = %d",
                run->steps_per_trial);
  COBEL_REQUIRE(run->trials >= 0 && run->trial_first >= 0 && run->trial_cap >= 0 &&
                    run->step_budget >= 0,
                COBEL_E_RANGE, "cobel_anet_run: trials = %d, trial_first = %d, trial_cap = %d",
                run->trials, run->trial_first, run->trial_cap);
  COBEL_REQUIRE((run->trace == nullptr) == (run->trace_len == nullptr) &&
                    (!run->trace || run->trace_cap >= 0),
                COBEL_E_ARG, "cobel_anet_run: trace and trace_len go together");
  COBEL_REQUIRE((((uintptr_t)run->eps | (uintptr_t)run->trew | (uintptr_t)run->trial_reward |
                  (uintptr_t)run->trace | (uintptr_t)run->steps_done) & 7u) == 0 &&
                    (((uintptr_t)run->pol_ctr | (uintptr_t)run->agent_ctr |
                      (uintptr_t)run->instance_ids | (uintptr_t)run->mid |
                      (uintptr_t)run->trial_steps | (uintptr_t)run->trial_action |
                      (uintptr_t)run->trace_len) & 3u) == 0,
                COBEL_E_ARG, "cobel_anet_run: misaligned argument");
  if (seq->n == 0 || run->trials == 0) return COBEL_OK;
  anet_args K;
  K.s = *seq;
  K.r = *run;
  K.G = group_lanes(seq->dim);
  COBEL_HIP_TRY(cobel_launch(k_anet_run, dim3(group_blocks(seq->n, K.G)), dim3(64 * kWaves), 0,
                             (hipStream_t)stream, K));
  return COBEL_OK;
}

extern "C" int cobel_anet_predict(const cobel_anet_run_t* run, int32_t dim, const double* batch,
                                  int32_t n_batch, double* out, void* stream) {
  if (int rc = check_weights(run, "cobel_anet_predict")) return rc;
  if (int rc = check_shape(dim, run->n_actions, run->n, "cobel_anet_predict")) return rc;
  COBEL_REQUIRE(n_batch >= 0, COBEL_E_RANGE, "cobel_anet_predict: batch of %d", n_batch);
  COBEL_REQUIRE(run->agent_ctr && ((uintptr_t)run->agent_ctr & 3u) == 0 &&
                    ((uintptr_t)run->instance_ids & 3u) == 0,
                COBEL_E_ARG, "cobel_anet_predict: agent_ctr must be given, aligned");
  if (run->n == 0 || n_batch == 0) return COBEL_OK;
  COBEL_REQUIRE(batch && out, COBEL_E_ARG, "cobel_anet_predict: NULL argument");
  COBEL_REQUIRE((((uintptr_t)batch | (uintptr_t)out) & 7u) == 0, COBEL_E_ARG,
                "cobel_anet_predict: misaligned argument");
  COBEL_REQUIRE((long long)run->n * n_batch <= 0x7fffffffll / COBEL_ANET_MAX_ACTIONS, COBEL_E_RANGE,
                "cobel_anet_predict: %d instances x %d rows", run->n, n_batch);
  const int G = group_lanes(dim);
  hipLaunchKernelGGL(k_anet_predict, dim3(group_blocks((long long)run->n * n_batch, G)),
                     dim3(64 * kWaves), 0, (hipStream_t)stream, *run, dim, G, batch, n_batch, out);
  COBEL_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_anet_advance, dim3((unsigned)((run->n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, run->agent_ctr, run->n,
                     (uint32_t)n_batch * (uint32_t)(run->n_actions - 1));
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_anet_update(const cobel_anet_run_t* run, int32_t dim, const double* state,
                                 const int32_t* action, const double* reward, void* stream) {
  if (int rc = check_weights(run, "cobel_anet_update")) return rc;
  if (int rc = check_shape(dim, run->n_actions, run->n, "cobel_anet_update")) return rc;
  if (int rc = check_rates(run, "cobel_anet_update")) return rc;
  if (run->n == 0) return COBEL_OK;
  COBEL_REQUIRE(state && action && reward, COBEL_E_ARG, "cobel_anet_update: NULL argument");
  COBEL_REQUIRE((((uintptr_t)state | (uintptr_t)reward) & 7u) == 0 && ((uintptr_t)action & 3u) == 0,
                COBEL_E_ARG, "cobel_anet_update: misaligned argument");
  const long long lanes = (long long)run->n * dim;
  hipLaunchKernelGGL(k_anet_update, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, *run, dim, state, action, reward);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
