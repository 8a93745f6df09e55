// A session on a cobel_tab_run_t, said once: the world as a kernel sees it, the instance record
// (inst[COBEL_I_*]) as registers, the trial protocol — start from the env stream, the five monitors
// at the end — and the small stores every kernel makes the same way; on the host the argument
// checks of a run and the instances-per-workgroup chooser of the wavefront kernels with LDS tables.
//
// The formats and the order of effects below are a contract: a session may be cut at any step and
// go on in another kernel (tests/test_gpu_tab_handover.py).  k_tab_general and k_tab_rollout are
// written on these pieces.  The tuned kernels (tabular.hip, tabular_nact.hip, tabular_pwg.hip,
// sr*.hip, ...) and k_tab_pol (tabular_policy.hip: on these pieces it measured 1 % slower) still
// spell the same protocol out by hand and must agree with it; their hosts use the checks below.
#pragma once
#include "cobel_common.h"

// ---- the world ----------------------------------------------------------------------------------
// First member of a kernel's argument struct.  `wbase` is world * S.
struct cobel_world_view {
  const cobel_wrec* rec;        // four-action worlds
  const uint16_t* next_n;       // other action counts: [W][S][A]
  const float* reward_s;        // [W][S]
  const uint8_t* terminal_s;    // [W][S]
  const uint16_t* starts;
  const int32_t* start_off;
  // transition rows that are distributions (cobel_world_set_transitions), or NULL
  const uint32_t* succ_off;
  const uint16_t* succ_state;
  const double* succ_cdf;
  int32_t S, n_worlds, A;

  __device__ __forceinline__ int next(size_t wbase, int s, int a) const {
    return rec ? (int)rec[wbase + s].next[a] : (int)next_n[(wbase + s) * A + a];
  }
  __device__ __forceinline__ float reward(size_t wbase, int s) const {
    return rec ? rec[wbase + s].reward : reward_s[wbase + s];
  }
  __device__ __forceinline__ uint32_t terminal(size_t wbase, int s) const {
    return rec ? rec[wbase + s].terminal : (uint32_t)terminal_s[wbase + s];
  }
  // where succ_off is set: the successor drawn from the row of (s, a) for the uniform u
  // (interface/gridworld.py:119-123)
  __device__ __forceinline__ int drawn_next(size_t wbase, int s, int a, double u) const {
    return cobel_draw_successor(succ_off, succ_state, succ_cdf, (wbase + (size_t)s) * A + a, u);
  }
};

inline cobel_world_view cobel_world_view_of(const cobel_world* world) {
  return {world->rec,       world->next_n,   world->reward_s,   world->terminal_s,
          world->starts,    world->start_off, world->succ_off,  world->succ_state,
          world->succ_cdf,  world->n_states, world->n_worlds,   world->n_actions};
}

#if defined(__HIPCC__)
// ---- the monitors of a finished trial --------------------------------------------------------------
// RUN: any run struct (they name these members alike).  One caller per instance: a kernel with
// several lanes per instance guards the call.
template <typename RUN>
__device__ __forceinline__ void cobel_trial_monitor(const RUN& run, int i, int trial, int latency,
                                                    double trew) {
  if (trial >= 0 && trial < run.trial_cap) {
    const size_t m = cobel_mon_offset(run.mon_stripes, run.trial_cap) + (size_t)trial;
    if (run.lat_sum) atomicAdd(run.lat_sum + m, (unsigned long long)latency);
    if (run.lat_cnt) atomicAdd(run.lat_cnt + m, 1ull);
    if (run.reward_sum) atomicAdd(run.reward_sum + m, trew);
    if (run.resp_cnt && trew > 0.0) atomicAdd(run.resp_cnt + m, 1ull);
    if (run.lat_trace) run.lat_trace[(size_t)i * run.trial_cap + trial] = latency;
  }
}

// ---- the instance record ----------------------------------------------------------------------------
struct cobel_tab_session {
  int state, step, trial;
  uint32_t ce, cp, cm, loglen, iflags;   // the stream counters, the log length, bit 0: in a trial
  double trew;
  unsigned long long executed, batches;  // of this call
  int start_lo;                          // the starting states of the instance's world
  uint32_t start_cnt;

  // (raw: a kernel that indexes LDS by the state clamps it where it loads)
  __device__ __forceinline__ void load(const int32_t* inst, const cobel_world_view& W, int world) {
    state = inst[COBEL_I_STATE];
    step = inst[COBEL_I_STEP];
    trial = inst[COBEL_I_TRIAL];
    ce = (uint32_t)inst[COBEL_I_CTR_ENV];
    cp = (uint32_t)inst[COBEL_I_CTR_POLICY];
    cm = (uint32_t)inst[COBEL_I_CTR_MEMORY];
    loglen = (uint32_t)inst[COBEL_I_LOG_LEN];
    iflags = (uint32_t)inst[COBEL_I_FLAGS];
    trew = *reinterpret_cast<const double*>(inst + COBEL_I_REWARD_LO);
    executed = batches = 0ull;
    start_lo = W.start_off[world];
    start_cnt = (uint32_t)(W.start_off[world + 1] - start_lo);
  }
  // memory: false in a session that neither replays nor logs — the memory counter, the log length
  // and batches_done stay as they are (and cost such a kernel no registers)
  template <typename RUN>
  __device__ __forceinline__ void store(int32_t* inst, const RUN& run, bool memory = true) const {
    inst[COBEL_I_STATE] = state;
    inst[COBEL_I_STEP] = step;
    inst[COBEL_I_TRIAL] = trial;
    inst[COBEL_I_CTR_ENV] = (int32_t)ce;
    inst[COBEL_I_CTR_POLICY] = (int32_t)cp;
    if (memory) {
      inst[COBEL_I_CTR_MEMORY] = (int32_t)cm;
      inst[COBEL_I_LOG_LEN] = (int32_t)loglen;
    }
    inst[COBEL_I_FLAGS] = (int32_t)iflags;
    *reinterpret_cast<double*>(inst + COBEL_I_REWARD_LO) = trew;
    *reinterpret_cast<unsigned long long*>(inst + COBEL_I_STEPS_LO) += executed;
    if (run.steps_done && executed) atomicAdd(run.steps_done, executed);
    if (memory && run.batches_done && batches) atomicAdd(run.batches_done, batches);
  }

  // Outside a trial (bit 0 of iflags clear): the session is over once trials_target trials are done,
  // else the next trial starts at a state drawn from the env stream (g: the instance's global id).
  // (Two calls, the test at the caller's `break`: as ONE call that returns false k_tab_rollout takes
  //  nine more vector registers in every instantiation and loses a wave of occupancy in two.)
  template <typename RUN>
  __device__ __forceinline__ bool done(const RUN& run) const { return trial >= run.trials_target; }
  template <typename RUN>
  __device__ __forceinline__ void begin_trial(const cobel_world_view& W, const RUN& run, uint32_t g) {
    state = (int)W.starts[start_lo + (int)cobel_draw_bounded(ce, 0u, g, COBEL_STREAM_ENV, run.seed,
                                                             start_cnt)];
    ce += 1u;
    step = 0;
    trew = 0.0;
    iflags |= 1u;
  }
  // report: false on all lanes but one where several lanes hold the instance
  template <typename RUN>
  __device__ __forceinline__ void end_trial(const RUN& run, int i, bool report = true) {
    if (report) cobel_trial_monitor(run, i, trial, step, trew);
    trial += 1;
    iflags &= ~1u;
  }
};

// the policy stream of a run
__device__ __forceinline__ uint32_t cobel_policy_stream(uint32_t flags) {
  return (flags & COBEL_F_TEST_STREAM) ? COBEL_STREAM_POLICY_TEST : COBEL_STREAM_POLICY;
}

// instance i's parameter set (param_index[i], clamped to the sets there are), or NULL
template <typename RUN>
__device__ __forceinline__ const cobel_param_set_t* cobel_pick_param_set(const RUN& run, int i) {
  if (!run.param_index) return nullptr;
  const int k = (int)run.param_index[i];
  return run.param_sets + (k < run.n_param_sets ? k : run.n_param_sets - 1);
}

// Dyna-Q's model store in float32 (memory/dyna_q.py:92-96) with its digest word; returns the record
__device__ __forceinline__ uint64_t cobel_model_store_f32(uint64_t* model, uint16_t* mindex,
                                                          size_t sa, float r, uint32_t ns,
                                                          uint32_t nt, float mlr_f) {
  const float R = __builtin_bit_cast(float, (uint32_t)model[sa]);
  const float d = r - R;
  const float Rn = R + mlr_f * d;
  const uint64_t rec = cobel_model_pack(Rn, ns, nt);
  model[sa] = rec;
  if (mindex)
    mindex[sa] = (uint16_t)(ns | (nt << 14) | (__builtin_bit_cast(uint32_t, Rn) ? 0x8000u : 0u));
  return rec;
}

// last_exp[i] = {s, a, ns, nonterminal, f32 r, f32 td}
__device__ __forceinline__ void cobel_last_exp_store(int32_t* last_exp, int i, int s, int a, int ns,
                                                     uint32_t nt, float r, float td) {
  int32_t* const e = last_exp + (size_t)i * 6;
  e[0] = s;
  e[1] = a;
  e[2] = ns;
  e[3] = (int32_t)nt;
  e[4] = __builtin_bit_cast(int32_t, r);
  e[5] = __builtin_bit_cast(int32_t, td);
}
#endif

// ---- host: the checks of a run that read only the arguments -------------------------------------
// `what`: the clauses the entry points do not share.  Never touches a device; world is not NULL.
enum : unsigned {
  COBEL_CHECK_EPSILON = 1u,      // epsilon is a parameter of the run
  COBEL_CHECK_Q_ROWS16 = 2u,     // rows of four values are read as one 16-byte load
  COBEL_CHECK_TABLES = 4u,       // the run may learn: agent, model, log, batch, steps, caps
  COBEL_CHECK_DIGEST_WORD = 8u,  // model_index is read as 64-bit words of four digests
};

inline int cobel_tab_run_check(const cobel_world* world, const cobel_tab_run_t& r, const char* who,
                               unsigned what) {
  const int A = world->n_actions;
  const bool rows16 = (what & COBEL_CHECK_Q_ROWS16) != 0;
  COBEL_REQUIRE(r.q && r.inst, COBEL_E_ARG, "%s: q and inst are required", who);
  COBEL_REQUIRE(((uintptr_t)r.q & (rows16 && A == 4 ? 15u : 3u)) == 0 &&
                    ((uintptr_t)r.inst & 7u) == 0, COBEL_E_ARG,
                "%s: q must be %d-byte and inst 8-byte aligned", who, rows16 ? 16 : 4);
  if (what & COBEL_CHECK_TABLES) {
    const int digest = (what & COBEL_CHECK_DIGEST_WORD) ? 8 : 2;
    COBEL_REQUIRE(((uintptr_t)r.model & 7u) == 0 && ((uintptr_t)r.replay_log & 7u) == 0,
                  COBEL_E_ARG, "%s: model and replay_log must be 8-byte aligned", who);
    COBEL_REQUIRE(((uintptr_t)r.model_index & (uintptr_t)(digest - 1)) == 0, COBEL_E_ARG,
                  "%s: model_index must be %d-byte aligned", who, digest);
  }
  COBEL_REQUIRE(r.n >= 0, COBEL_E_RANGE, "%s: n = %d", who, r.n);
  if (what & COBEL_CHECK_TABLES) {
    COBEL_REQUIRE(r.agent == COBEL_AGENT_Q || r.agent == COBEL_AGENT_DYNAQ, COBEL_E_ARG,
                  "%s: unknown agent %d", who, r.agent);
    COBEL_REQUIRE(r.agent != COBEL_AGENT_DYNAQ || r.model, COBEL_E_ARG,
                  "%s: Dyna-Q needs the model table", who);
    COBEL_REQUIRE(r.batch >= 0, COBEL_E_RANGE, "%s: batch %d", who, r.batch);
    COBEL_REQUIRE(r.steps_per_trial > 0, COBEL_E_RANGE, "%s: steps_per_trial = %d", who,
                  r.steps_per_trial);
    COBEL_REQUIRE(r.trial_cap >= 0 && r.log_cap >= 0, COBEL_E_RANGE, "%s: negative cap", who);
  }
  if (what & COBEL_CHECK_EPSILON)
    COBEL_REQUIRE(r.epsilon >= 0.0 && r.epsilon <= 1.0, COBEL_E_ARG, "%s: epsilon %g outside [0, 1]",
                  who, r.epsilon);
  COBEL_REQUIRE(!(r.flags & COBEL_F_MASK_ACTIONS) || r.action_mask, COBEL_E_ARG,
                "%s: mask_actions set without an action mask", who);
  COBEL_REQUIRE(A <= 8 || !(r.flags & COBEL_F_MASK_ACTIONS) || ((uintptr_t)r.action_mask & 3u) == 0,
                COBEL_E_ARG, "%s: the action masks of a %d-action world are 32-bit words, 4-byte "
                "aligned", who, A);
  COBEL_REQUIRE(!r.param_index || (r.param_sets && r.n_param_sets > 0), COBEL_E_ARG,
                "%s: param_index given without parameter sets", who);
  return COBEL_OK;
}

// ---- host: instances per workgroup of a wavefront kernel with its tables in LDS -------------------
// Instances per workgroup where they share the world's copy: the count (1, 2, 4 or 8) that puts the
// most wavefronts on a CU — up to four unless eight win (k_tab_wqn, rows of 16 on 256 states: 17.5 KB
// per instance + 11 KB of world and masks, eight in ONE workgroup where two workgroups of four miss
// the 160 KiB by 2 KB and three of two make six).  With few instances rather a workgroup on every CU
// than full workgroups on a few of them.  lds_of_wpg(w): the LDS of a workgroup of w instances.
template <typename LdsBytes>
int cobel_wave_plan(size_t lds_cu, int n_cu, int n, bool shared, LdsBytes lds_of_wpg) {
  int wpg = 1;
  if (shared) {
    size_t best = 0;
    for (int w = 1; w <= 8; w <<= 1) {
      const size_t need = lds_of_wpg(w);
      if (need > lds_cu) break;
      size_t waves = (lds_cu / need) * (size_t)w;
      if (waves > 16) waves = 16;
      if (waves > best || (waves == best && w <= 4)) {
        best = waves;
        wpg = w;
      }
    }
  }
  while (wpg > 1 && (n + wpg - 1) / wpg < n_cu) wpg >>= 1;
  return wpg;
}
