// What the kernels on a Sequence environment share (rw.hip, anet.hip): the packing of instances
// into lane groups, the fixed summation tree inside a group, and the playback of a schedule
// (interface/sequence.py:129-204) from the tables of a cobel_seq_t.
#pragma once
#include "cobel_common.h"

namespace cobel_seq {

constexpr int kWaves = 4;   // wavefronts per workgroup

// Balanced binary tree over the G lanes of a group (G a power of two), adjacent leaves first;
// every lane of the group ends with the same bits.  To be called in wave-uniform control flow.
__device__ __forceinline__ double group_sum(double p, int G) {
  for (int o = 1; o < G; o <<= 1) p = p + __shfl_xor(p, o);
  return p;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The trial offsets of instance i's schedule
__device__ __forceinline__ const int32_t* trial_offsets(const cobel_seq_t& S, int i) {
  const int sched = clampi(S.schedule_of ? S.schedule_of[i] : 0, 0, S.n_schedules - 1);
  return S.trial_off + (size_t)sched * (S.n_trials + 1);
}

// The schedule step at (current_trial, current_step), both clamped before use (a lane that is not
// alive still loads, from an element that exists); len: the steps of that trial
__device__ __forceinline__ int step_at(const cobel_seq_t& S, const int32_t* toff, int ct, int cs,
                                       int& base, int& len) {
  const int tc = clampi(ct, 0, S.n_trials - 1);
  base = toff[tc];
  len = toff[tc + 1] - base;
  return clampi(base + clampi(cs, 0, len - 1), 0, S.n_steps - 1);
}

// The reward of schedule step `at` for `action` (sequence.py:157-166): the float, or the entry of
// the array the action — the step's own under overwrite — selects
__device__ __forceinline__ double step_reward(const cobel_seq_t& S, int at, int action) {
  const int A = S.n_actions;
  if (S.step_scalar[at]) return S.step_reward[(size_t)at * A];
  const int forced = S.step_action[at];
  const int a = clampi((S.overwrite && forced >= 0) ? forced : action, 0, A - 1);
  return S.step_reward[(size_t)at * A + a];
}

inline int group_lanes(int dim) {
  int G = 1;
  while (G < dim) G <<= 1;
  return G;
}

inline unsigned group_blocks(long long groups, int G) {
  const long long per_block = (long long)kWaves * (64 / G);
  return (unsigned)((groups + per_block - 1) / per_block);
}

inline int check_seq(const cobel_seq_t* s, const char* who) {
  COBEL_REQUIRE(s, COBEL_E_ARG, "%s: NULL sequence", who);
  COBEL_REQUIRE(s->dim >= 1 && s->dim <= COBEL_RW_MAX_DIM, COBEL_E_UNSUPPORTED,
                "%s: observations of %d components (a Sequence serves 1 to %d)", who, s->dim,
                COBEL_RW_MAX_DIM);
  COBEL_REQUIRE(s->n >= 0, COBEL_E_RANGE, "%s: n = %d", who, s->n);
  COBEL_REQUIRE(s->n_obs >= 1 && s->n_actions >= 1 && s->n_schedules >= 1 && s->n_trials >= 1 &&
                    s->n_steps >= s->n_trials,
                COBEL_E_RANGE,
                "%s: %d observation rows, %d actions, %d schedules of %d trials, %d steps", who,
                s->n_obs, s->n_actions, s->n_schedules, s->n_trials, s->n_steps);
  COBEL_REQUIRE(s->obs_table && s->step_obs && s->step_action && s->step_scalar && s->step_reward &&
                    s->trial_off && s->cur_trial && s->cur_step,
                COBEL_E_ARG, "%s: NULL table", who);
  COBEL_REQUIRE((((uintptr_t)s->obs_table | (uintptr_t)s->step_reward) & 7u) == 0 &&
                    (((uintptr_t)s->step_obs | (uintptr_t)s->step_action | (uintptr_t)s->trial_off |
                      (uintptr_t)s->schedule_of | (uintptr_t)s->cur_trial |
                      (uintptr_t)s->cur_step) & 3u) == 0,
                COBEL_E_ARG, "%s: misaligned table", who);
  return COBEL_OK;
}

}  // namespace cobel_seq
