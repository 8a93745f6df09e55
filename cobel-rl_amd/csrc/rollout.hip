// A test session that records (cobel_tab_rollout): the trial loop of a run that does not learn,
// restated once more with the stores of a trajectory record in it.
//
// One LANE per instance, as k_tab_general: nothing learns, so no table has to live in LDS — a lane
// reads the Q row of its state from device memory (one 16-byte load in four-action worlds) and the
// world record of the state it enters.  Without LDS a SIMD can hold many waves to cover those
// dependent gathers, so small launches go out in narrow workgroups (cobel_tab_general_plan's rule).
// Streams, counters, selection (cobel_eps_greedy_select_n: float64 probabilities, ties by exact
// float32 equality), the successor draw and the monitors are k_tab_general's with COBEL_F_LEARN
// clear, which the wavefront kernels reproduce bit for bit: a session run here leaves what
// cobel_tab_run leaves.
//
// The record.  Rows are [N][trials * steps]: each lane writes a sequential stream of 2-byte states
// and 1-byte actions.  A store per entry would be two requests of one sector each per lane and
// step — as many again as the step's two loads.  A lane keeps four steps in registers instead
// (an aligned group of four entries: 8 bytes of states, 4 of actions) and writes a full group as
// one 8-byte and one 4-byte store; the entries of a group a trial fills only in part — at most
// three at its head, three at its tail — go out one by one, so nothing outside a trial's own
// entries is ever written.  The padding (0xff bytes) is a plain fill of both arrays before the
// launch.  COBEL_ROLLOUT_ELEMENT_STORES keeps the store per entry for comparison.
#include "cobel_common.h"
#include "cobel_policy.h"
#include "cobel_tab_session.h"

namespace {

struct rollout_args {
  cobel_world_view w;
  cobel_tab_rollout_t o;
};

template <int AMAX>
__device__ __forceinline__ uint32_t rollout_mask(const uint8_t* mask, int s) {
  if (!mask) return 0xffffffffu;
  if (AMAX > 8) return reinterpret_cast<const uint32_t*>(mask)[s];
  return (uint32_t)mask[s];
}

// AMAX 4: four-action worlds, rows read as one float4; 8 / 16 / 32: the other action counts.
template <int AMAX>
__global__ __launch_bounds__(64) void k_tab_rollout(const rollout_args G) {
  const cobel_tab_run_t& R = G.o.run;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= R.n) return;
  const cobel_world_view& W = G.w;
  const int S = W.S, A = W.A;
  const uint32_t g = R.instance_base + (uint32_t)i;
  const int world = (int)(g % (uint32_t)W.n_worlds);
  const size_t wbase = (size_t)world * S;
  const float* const Q = R.q + (size_t)i * S * A;

  int32_t* const inst = R.inst + (size_t)i * COBEL_I_WORDS;
  cobel_tab_session X;
  X.load(inst, W, world);
  X.state = min(max(X.state, 0), S - 1);

  const uint32_t flags = R.flags;
  const uint32_t pol_stream = cobel_policy_stream(flags);
  const uint8_t* const amask = (flags & COBEL_F_MASK_ACTIONS) ? R.action_mask : nullptr;
  const uint64_t seed = R.seed;
  double eps = R.epsilon;
  if (const cobel_param_set_t* const P = cobel_pick_param_set(R, i)) eps = P->epsilon;

  // the record: session trial t = trial - first, entry e = (i * trials + t) * steps + step
  const int trials = G.o.trials, steps = G.o.steps;
  const int first = R.trials_target - trials;
  const bool wide = !(G.o.record_flags & COBEL_ROLLOUT_ELEMENT_STORES);
  uint64_t sacc = 0;     // the staged entries of the group e0 >> 2, each at its slot e & 3
  uint32_t aacc = 0;
  size_t e0 = 0;
  int fill = 0;
  auto flush = [&]() {
    if (fill == 4 && wide) {   // (four consecutive entries ending at slot 3: e0 is a multiple of 4)
      *reinterpret_cast<uint64_t*>(G.o.states + e0) = sacc;
      *reinterpret_cast<uint32_t*>(G.o.actions + e0) = aacc;
    } else {
      for (int j = 0; j < fill; ++j) {
        const size_t e = e0 + (size_t)j;
        const int slot = (int)(e & 3u);
        G.o.states[e] = (int16_t)(uint16_t)(sacc >> (16 * slot));
        G.o.actions[e] = (uint8_t)(aacc >> (8 * slot));
      }
    }
    sacc = 0;
    aacc = 0;
    fill = 0;
  };

  while (true) {
    if (!(X.iflags & 1u)) {
      if (X.done(R)) break;
      X.begin_trial(W, R, g);
      if ((unsigned)(X.trial - first) < (unsigned)trials)
        G.o.start[(size_t)i * trials + (X.trial - first)] = (int16_t)X.state;
    }

    // ---- select + env.step ----------------------------------------------------------------------
    float qv[AMAX];
    if (AMAX == 4) {
      const float4 row = reinterpret_cast<const float4*>(Q)[X.state];
      qv[0] = row.x;
      qv[1] = row.y;
      qv[2] = row.z;
      qv[3] = row.w;
    } else {
#pragma unroll
      for (int a = 0; a < AMAX; ++a) qv[a] = a < A ? Q[(size_t)X.state * A + a] : 0.0f;
    }
    const double u = cobel_draw_u01(X.cp, 0u, g, pol_stream, seed);
    X.cp += 1u;
    const int a = cobel_eps_greedy_select_n<float, AMAX>(qv, A, rollout_mask<AMAX>(amask, X.state),
                                                         u, eps, nullptr);
    int ns;
    if (W.succ_off) {   // the successor is drawn from the row (gridworld.py:119-123)
      const double ue = cobel_draw_u01(X.ce, COBEL_SUB_DOUBLE, g, COBEL_STREAM_ENV, seed);
      X.ce += 1u;
      ns = W.drawn_next(wbase, X.state, a, ue);
    } else {
      ns = W.next(wbase, X.state, a);
    }
    const float r = W.reward(wbase, ns);
    const uint32_t end = W.terminal(wbase, ns);
    X.trew += (double)r;
    X.executed += 1ull;
    if (R.occupancy) atomicAdd(R.occupancy + wbase + ns, 1ull);
    const bool trial_over = end || (X.step + 1 >= R.steps_per_trial);

    // ---- the record -----------------------------------------------------------------------------
    const bool in_record =
        (unsigned)(X.trial - first) < (unsigned)trials && (unsigned)X.step < (unsigned)steps;
    if (in_record) {
      const size_t e = ((size_t)i * trials + (size_t)(X.trial - first)) * steps + (size_t)X.step;
      const int slot = (int)(e & 3u);
      if (fill == 0) e0 = e;
      sacc |= (uint64_t)(uint16_t)ns << (16 * slot);
      aacc |= (uint32_t)(uint8_t)a << (8 * slot);
      fill += 1;
      if (!wide || slot == 3) flush();
    }
    X.state = ns;

    if (trial_over) {
      if (fill) flush();
      if (in_record) G.o.length[(size_t)i * trials + (X.trial - first)] = X.step + 1;
      X.end_trial(R, i);
    } else {
      X.step += 1;
    }
  }

  X.store(inst, R, false);   // (a rollout has no memory: those words are not written)
}

__global__ __launch_bounds__(256) void k_rollout_visits(const int16_t* __restrict__ states,
                                                        size_t total, size_t per_instance, int S,
                                                        int n_worlds, uint32_t base,
                                                        unsigned long long* __restrict__ counts) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int s = (int)states[e];
  if (s < 0 || s >= S) return;
  const uint32_t g = base + (uint32_t)(e / per_instance);
  atomicAdd(counts + (size_t)(g % (uint32_t)n_worlds) * S + s, 1ull);
}

// The checks of both entry points and the shape of the launch: out = {LDS bytes, threads per
// workgroup, instances per workgroup, workgroups}.  What reads only the arguments comes before what
// asks the runtime for the current device.
int rollout_plan(const cobel_world_t* world, const cobel_tab_rollout_t* o, int32_t out[4],
                 const char* who) {
  out[0] = out[1] = out[2] = out[3] = 0;
  COBEL_REQUIRE(world && o, COBEL_E_ARG, "%s: NULL world/rollout", who);
  const cobel_tab_run_t& r = o->run;
  COBEL_REQUIRE(o->start && o->states && o->actions && o->length, COBEL_E_ARG,
                "%s: the record needs start, states, actions and length", who);
  COBEL_REQUIRE(!(r.flags & COBEL_F_LEARN), COBEL_E_ARG,
                "%s: COBEL_F_LEARN is set: a rollout is a test session, it never writes Q", who);
  COBEL_REQUIRE(r.step_budget == 0, COBEL_E_ARG,
                "%s: step_budget = %d: a rollout runs whole sessions (step_budget 0)", who,
                r.step_budget);
  COBEL_REQUIRE(o->trials >= 1 && o->steps >= 1, COBEL_E_RANGE, "%s: trials = %d, steps = %d", who,
                o->trials, o->steps);
  COBEL_REQUIRE(r.steps_per_trial == o->steps, COBEL_E_ARG,
                "%s: steps_per_trial = %d, the record keeps %d steps per trial", who,
                r.steps_per_trial, o->steps);
  COBEL_REQUIRE(r.trials_target >= o->trials, COBEL_E_RANGE,
                "%s: trials_target %d is below the session's %d trials", who, r.trials_target,
                o->trials);
  COBEL_REQUIRE(r.trial_cap >= r.trials_target, COBEL_E_RANGE,
                "%s: trial_cap %d is too small for trials_target %d", who, r.trial_cap,
                r.trials_target);
  COBEL_REQUIRE(world->n_actions >= 1 && world->n_actions <= COBEL_MAX_ACTIONS, COBEL_E_UNSUPPORTED,
                "%s: %d actions (1..%d are served)", who, world->n_actions, COBEL_MAX_ACTIONS);
  COBEL_REQUIRE(((uintptr_t)r.q & (world->n_actions == 4 ? 15u : 3u)) == 0, COBEL_E_ARG,
                "%s: q is misaligned: rows of %d float32 values must be %d-byte aligned", who,
                world->n_actions, world->n_actions == 4 ? 16 : 4);
  COBEL_REQUIRE(((uintptr_t)o->states & 7u) == 0 && ((uintptr_t)o->actions & 3u) == 0 &&
                    ((uintptr_t)o->start & 1u) == 0 && ((uintptr_t)o->length & 3u) == 0,
                COBEL_E_ARG, "%s: the record is misaligned (states 8, actions 4, start 2, length 4 "
                "bytes)", who);
  // (a rollout reads neither the agent kind nor the model, the log or the batch of its run; q's
  //  alignment was refused above in this entry point's own words, so of the shared q / inst clause
  //  only the inst half can still fire)
  if (int rc = cobel_tab_run_check(world, r, who, COBEL_CHECK_EPSILON | COBEL_CHECK_Q_ROWS16))
    return rc;
  if (int rc = cobel_world_check(world, who)) return rc;
  if (r.n == 0) return COBEL_OK;
  cobel_tab_plan P{};
  cobel_tab_general_plan(r, P);   // lanes per workgroup: narrow workgroups for small launches
  out[0] = 0;
  out[1] = P.lpb;
  out[2] = P.lpb;
  out[3] = (r.n + P.lpb - 1) / P.lpb;
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_tab_rollout_plan(const cobel_world_t* world, const cobel_tab_rollout_t* rollout,
                                      int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_tab_rollout_plan: NULL out");
  return rollout_plan(world, rollout, out, "cobel_tab_rollout_plan");
}

extern "C" int cobel_tab_rollout(const cobel_world_t* world, const cobel_tab_rollout_t* rollout,
                                 void* stream) {
  int32_t plan[4];
  if (int rc = rollout_plan(world, rollout, plan, "cobel_tab_rollout")) return rc;
  if (!plan[3]) return COBEL_OK;   // n == 0
  hipStream_t st = (hipStream_t)stream;
  rollout_args G;
  G.w = cobel_world_view_of(world);
  G.o = *rollout;
  const size_t entries = (size_t)rollout->run.n * (size_t)rollout->trials * (size_t)rollout->steps;
  COBEL_HIP_TRY(hipMemsetAsync(rollout->states, 0xff, entries * sizeof(int16_t), st));
  COBEL_HIP_TRY(hipMemsetAsync(rollout->actions, 0xff, entries, st));
  void (*kernel)(const rollout_args) = &k_tab_rollout<32>;
  if (G.w.A == 4) kernel = &k_tab_rollout<4>;
  else if (G.w.A <= 8) kernel = &k_tab_rollout<8>;
  else if (G.w.A <= 16) kernel = &k_tab_rollout<16>;
  COBEL_HIP_TRY(cobel_launch(kernel, dim3((unsigned)plan[3]), dim3((unsigned)plan[1]), 0, st, G));
  return COBEL_OK;
}

extern "C" int cobel_rollout_visits(const int16_t* states, int32_t n, int64_t per_instance,
                                    int32_t n_states, int32_t n_worlds, uint32_t instance_base,
                                    unsigned long long* counts, void* stream) {
  COBEL_REQUIRE(states && counts, COBEL_E_ARG, "cobel_rollout_visits: NULL argument");
  COBEL_REQUIRE(n >= 0 && per_instance >= 1 && n_states >= 1 && n_states <= 16384 && n_worlds >= 1,
                COBEL_E_RANGE, "cobel_rollout_visits: n = %d, per_instance = %lld, n_states = %d, "
                "n_worlds = %d", n, (long long)per_instance, n_states, n_worlds);
  if (n == 0) return COBEL_OK;
  const size_t total = (size_t)n * (size_t)per_instance;
  COBEL_REQUIRE((total + 255) / 256 <= 0x7fffffffull, COBEL_E_RANGE,
                "cobel_rollout_visits: %zu entries are more than one launch takes", total);
  hipLaunchKernelGGL(k_rollout_visits, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, states, total, (size_t)per_instance, n_states, n_worlds,
                     instance_base, counts);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
