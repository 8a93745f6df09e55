// SFMA agent — one wavefront per agent–env instance (gfx950).
//
// SFMA is Dyna-Q whose replay picks experiences by priority R = C * D * (1 - I) [* T]: strength x
// similarity to the experience replayed last x (1 - inhibition) [x recency].  The reference
// evaluates R over all 4S experiences with NumPy for every single reactivation and draws one
// from softmax(R); that O(4S) scan + draw is the hot part (32 per trial by default).
//
// Here an instance's tables live in LDS for the whole call: Q (float32 [S][4]), strengths C
// (float64 [4S]), inhibition I (float64 [S]), the model's successor table NS (u16 [4S], experience
// order j = a * S + s, flag bit 15), its reward estimates R (float32 [4S]) and one scratch vector
// of 4S priorities.  Lane l owns the experiences
// [l * chunk, (l + 1) * chunk), so the cumulative sum behind the draw is one wave scan of lane
// totals plus a short in-lane running sum — element order as in the reference's cumsum.  The rows
// D[cur], D[next] of the similarity matrix (shared by all instances of a world, L2 resident) are
// staged in LDS once per reactivation.  The packed model records in HBM are written through on
// every store and never read back during the call; recency T is kept as a store stamp per experience and a
// table of decay powers instead of a vector that is rescaled on every store.
//
// Reference behaviour restated (paths relative to /root/reference/src/cobel):
//   agent/sfma.py:233-334 (train), :336-396 (test), :398-458 (replay, update_q)
//   memory/sfma.py:195-236 (store), :238-347 (replay), :349-372 (softmax), :374-416 (random batch)
#include "cobel_sfma.h"

using namespace cobel_sfma;

namespace {

template <int CH>
__global__ __launch_bounds__(64) void k_sfma(const sfma_args A) {
  sfma_body<CH, 1>(A);
}
// Two experiences per lane (worlds up to 32 states, the reference's demos): five waves per SIMD
// instead of the four the register allocation settles on by itself — +12 % on C6 —, six for the
// plain-training instantiation since the constants of the masked action selection and the ones a
// reactivation uses once (L.epsc) are read from LDS instead of being pinned to vector registers
// (80 registers, no scratch: +5 %; seven waves measure the same, eight 5 % less; 69 registers —
// seven waves resident — since the LDS layout is fixed at compile time).  The same hint
// costs the wider variants 20-25 % (spills into scratch), so they keep the default.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_sfma_2(
    const sfma_args A) {
  sfma_body<2, 1>(A);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_sfma_2_fast(
    const sfma_args A) {
  sfma_body<2, 1, true>(A);
}
// Four waves per instance, all switches: worlds of several hundred states.
__global__ __launch_bounds__(256) void k_sfma_wg(const sfma_args A) {
  sfma_body<0, 4>(A);
}

template <int CH>
int launch_sfma(const sfma_args& A, size_t lds, hipStream_t st) {
  const void* fn = CH == 2 ? reinterpret_cast<const void*>(&k_sfma_2)
                           : reinterpret_cast<const void*>(&k_sfma<CH>);
  if (lds > 64 * 1024)
    COBEL_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (CH == 2) hipLaunchKernelGGL(k_sfma_2, dim3(A.r.n), dim3(64), lds, st, A);
  else hipLaunchKernelGGL((k_sfma<CH>), dim3(A.r.n), dim3(64), lds, st, A);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
int launch_sfma_wg(const sfma_args& A, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024)
    COBEL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sfma_wg),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_sfma_wg, dim3(A.r.n), dim3(256), lds, st, A);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

}  // namespace

static const size_t kSfmaLdsLimit = 160 * 1024;

extern "C" int cobel_sfma_query(int32_t n_states, int32_t* lds_bytes) {
  COBEL_REQUIRE(n_states > 0, COBEL_E_RANGE, "cobel_sfma_query: %d states", n_states);
  const size_t lds = sfma_lds_bytes(n_states);
  if (lds_bytes) *lds_bytes = (int32_t)lds;
  COBEL_REQUIRE(lds <= kSfmaLdsLimit && n_states <= 16383, COBEL_E_UNSUPPORTED,
                "cobel_sfma_query: %d states need %zu B of LDS per instance (limit %zu)", n_states,
                lds, kSfmaLdsLimit);
  return COBEL_OK;
}

// One planner for describe (cobel_sfma_plan) and run (cobel_sfma_run): the form, the LDS of one
// workgroup, the threads of one instance and, for the streaming form, what it keeps in LDS.
//   form 0  LDS-resident, 128 B per state: S <= 1 274
//   form 1  streaming (sfma_big.hip); I always in LDS, then by room (160 KiB less 1 KiB fixed):
//           S <= 5 088   + Dc, Dn and the 2-byte successor table     32 B per state
//           S <= 6 784   + Dc, Dn                                    24 B per state
//           S <= 16 383  I alone, the similarity rows are read from `metric`    8 B per state
// (COBEL_DEBUG_SFMA_STREAM_LDS=<bytes> lowers the room of the streaming tiers, so that tests reach
//  every tier on small worlds; the choice between the two forms is not affected)
namespace {
struct sfma_plan {
  int form, lds, threads;
  uint32_t big_lds;
};
int sfma_plan_of(int32_t S, uint32_t flags, sfma_plan* P, const char* who) {
  COBEL_REQUIRE(S >= 1, COBEL_E_RANGE, "%s: %d states", who, S);
  COBEL_REQUIRE(S <= 16383, COBEL_E_UNSUPPORTED,
                "%s: %d states; the model keeps an experience's successor in a 15-bit field "
                "(NS | flag << 15), at most 16383 states",
                who, S);
  const size_t resident = sfma_lds_bytes(S);
  if (resident <= kSfmaLdsLimit && !(flags & COBEL_F_SFMA_STREAM)) {
    P->form = 0;
    P->lds = (int)resident;
    // (one wave per instance up to 800 experiences, four waves beyond: cobel_sfma_run)
    P->threads = (4 * S > 800 && !(flags & COBEL_F_NO_PREFETCH)) ? 256 : 64;
    P->big_lds = 0;
    return COBEL_OK;
  }
  size_t room = kSfmaLdsLimit;
  if (const char* const e = cobel_debug_env("COBEL_DEBUG_SFMA_STREAM_LDS")) {
    const long v = atol(e);
    if (v >= 4096 && (size_t)v <= kSfmaLdsLimit) room = (size_t)v;
  }
  uint32_t what = kBigNsInLds | kBigRowsInLds;
  if (sfma_big_lds_bytes(S, what) > room) what = kBigRowsInLds;
  if (sfma_big_lds_bytes(S, what) > room) what = 0;
  COBEL_REQUIRE(sfma_big_lds_bytes(S, what) <= kSfmaLdsLimit, COBEL_E_UNSUPPORTED,
                "%s: %d states need %zu B of LDS per instance (limit %zu)", who, S,
                sfma_big_lds_bytes(S, what), kSfmaLdsLimit);
  P->form = 1;
  P->lds = (int)sfma_big_lds_bytes(S, what);
  // 4S experiences over 256 threads up to 2 044 of them, over 1 024 beyond
  P->threads = S < 512 ? 256 : 1024;
  if (const char* const e = cobel_debug_env("COBEL_DEBUG_SFMA_STREAM_THREADS")) {   // (experiments)
    const long v = atol(e);
    if (v == 256 || v == 512 || v == 1024) P->threads = (int)v;
  }
  P->big_lds = what;
  return COBEL_OK;
}
}  // namespace

extern "C" int cobel_sfma_plan(int32_t n_states, uint32_t flags, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_sfma_plan: NULL out");
  sfma_plan P;
  if (int rc = sfma_plan_of(n_states, flags, &P, "cobel_sfma_plan")) return rc;
  out[0] = P.form;
  out[1] = P.lds;
  out[2] = P.threads;
  out[3] = 0;   // the streaming form rates its experiences again instead of keeping priorities
  return COBEL_OK;
}

namespace {
__global__ void k_exp_check(const double* x, double* a, double* b, const double* d, double* qa,
                            double* qb, int n) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e < n) {
    a[e] = exp_in_range(x[e]);
    b[e] = exp(x[e]);
    if (d) {
      qa[e] = quotient_by(x[e], d[e], 1.0 / d[e]);
      qb[e] = x[e] / d[e];
    }
  }
}
}  // namespace

extern "C" int cobel_sfma_exp_check(const double* x, double* in_range, double* library,
                                    const double* divisor, double* quotient_by_reciprocal,
                                    double* quotient, int32_t n, void* stream) {
  COBEL_REQUIRE(x && in_range && library && n >= 0 &&
                    (!divisor || (quotient_by_reciprocal && quotient)),
                COBEL_E_ARG, "cobel_sfma_exp_check: bad arguments");
  if (n == 0) return COBEL_OK;
  hipLaunchKernelGGL(k_exp_check, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x,
                     in_range, library, divisor, quotient_by_reciprocal, quotient, n);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_sfma_run(const cobel_world_t* world, const cobel_sfma_run_t* run,
                              void* stream) {
  if (int rc = cobel_world_check(world, "cobel_sfma_run")) return rc;
  COBEL_REQUIRE(world->n_actions == 4, COBEL_E_UNSUPPORTED,
                "cobel_sfma_run: the world has %d actions, this entry point serves four-action worlds",
                world->n_actions);
  COBEL_REQUIRE(world && run, COBEL_E_ARG, "cobel_sfma_run: NULL world/run");
  const cobel_sfma_run_t& r = *run;
  COBEL_REQUIRE(r.q && r.model && r.strength && r.stamp && r.inst && r.sfma_inst && r.metric,
                COBEL_E_ARG,
                "cobel_sfma_run: q, model, strength, stamp, inst, sfma_inst and metric are required");
  COBEL_REQUIRE(((uintptr_t)r.q & 15u) == 0 && ((uintptr_t)r.inst & 7u) == 0 &&
                    ((uintptr_t)r.sfma_inst & 7u) == 0 && ((uintptr_t)r.replay_trace & 7u) == 0,
                COBEL_E_ARG, "cobel_sfma_run: q must be 16-byte, inst / sfma_inst / trace 8-byte aligned");
  COBEL_REQUIRE(r.n >= 0, COBEL_E_RANGE, "cobel_sfma_run: n = %d", r.n);
  COBEL_REQUIRE(r.steps_per_trial > 0, COBEL_E_RANGE, "cobel_sfma_run: steps_per_trial = %d",
                r.steps_per_trial);
  COBEL_REQUIRE(r.batch >= 0 && r.nb_replays >= 0, COBEL_E_RANGE,
                "cobel_sfma_run: batch = %d, nb_replays = %d", r.batch, r.nb_replays);
  if (int rc = sfma_check_sets(r.param_sets, r.param_index, r.n_param_sets, "cobel_sfma_run"))
    return rc;
  // (with an index the scalars are ignored; a set's epsilon is checked where the set is filled)
  COBEL_REQUIRE(r.param_index || (r.epsilon >= 0.0 && r.epsilon <= 1.0), COBEL_E_ARG,
                "cobel_sfma_run: epsilon %g outside [0, 1]", r.epsilon);
  COBEL_REQUIRE(!(r.flags & COBEL_F_MASK_ACTIONS) || r.action_mask, COBEL_E_ARG,
                "cobel_sfma_run: mask_actions set without an action mask");
  COBEL_REQUIRE(!(r.sfma_flags & COBEL_SF_RANDOM) || r.random_cdf, COBEL_E_ARG,
                "cobel_sfma_run: random replay needs random_cdf");
  COBEL_REQUIRE(!(r.sfma_flags & COBEL_SF_RECENCY) || (r.recency_tab && r.recency_len > 0),
                COBEL_E_ARG, "cobel_sfma_run: recency needs recency_tab");
  COBEL_REQUIRE(!r.replay_trace || (r.trace_len && r.trace_cap > 0), COBEL_E_ARG,
                "cobel_sfma_run: replay_trace needs trace_len and trace_cap");
  const int S = world->n_states;
  sfma_plan P;
  if (int rc = sfma_plan_of(S, r.flags, &P, "cobel_sfma_run")) return rc;
  const int32_t lds = P.lds;
  if (r.n == 0) return COBEL_OK;
  sfma_args A;
  A.rec = world->rec;
  A.starts = world->starts;
  A.start_off = world->start_off;
  A.S = S;
  A.n_worlds = world->n_worlds;
  A.chunk = (4 * S + 63) / 64;
  A.r = r;
  const cobel_eps_consts ec = cobel_make_eps_consts(r.epsilon);
  for (int k = 0; k < 5; ++k) {
    A.eps.base[k] = ec.base[k];
    A.eps.bonus[k] = ec.bonus[k];
  }
  for (int k = 0; k < 16; ++k)
    for (int j = 0; j < 3; ++j) A.eps_thr[k][j] = ec.thr[k][j];
  A.alpha_f = (float)r.alpha;
  A.gamma_f = (float)r.gamma;
  A.model_lr_f = (float)r.model_lr;
  A.succ_off = world->succ_off;
  A.succ_state = world->succ_state;
  A.succ_cdf = world->succ_cdf;
  A.big_lds = P.big_lds;
  hipStream_t st = (hipStream_t)stream;
  if (P.form == 1) {
    COBEL_REQUIRE(((uintptr_t)r.strength & 15u) == 0 && ((uintptr_t)r.stamp & 15u) == 0 &&
                      ((uintptr_t)r.model & 7u) == 0,
                  COBEL_E_ARG,
                  "cobel_sfma_run: strength and stamp must be 16-byte, model 8-byte aligned");
    // (a multiple of four: the streaming form reads a thread's experiences four at a time)
    A.chunk = ((4 * S + P.threads - 1) / P.threads + 3) & ~3;
    return launch_sfma_big(A, P.threads, (size_t)P.lds, st);
  }
  const uint32_t special = COBEL_SF_RECENCY | COBEL_SF_C_NORMALIZE | COBEL_SF_D_NORMALIZE |
                           COBEL_SF_DETERMINISTIC;
  const bool plain = !(r.sfma_flags & special) && (r.sfma_flags & COBEL_SF_R_NORMALIZE) &&
                     !(r.flags & COBEL_F_FORCE_WAVE);
  if (plain && A.chunk <= 2) {
    A.chunk = 2;
    const uint32_t slow_sf = COBEL_SF_RANDOM | COBEL_SF_DYNAMIC | COBEL_SF_START_REPLAY |
                             COBEL_SF_REWARD_MOD_LOCAL | COBEL_SF_REWARD_MOD | COBEL_SF_STATE_MOD;
    const bool fast = (r.flags & COBEL_F_LEARN) &&
                      !(r.flags & (COBEL_F_NO_REPLAY | COBEL_F_TEST_STREAM)) &&
                      !(r.sfma_flags & slow_sf) && r.nb_replays == 1 && r.decay_strength == 1.0 &&
                      r.beta >= 0.0 && r.beta <= 700.0 && r.r_threshold >= 0.0 &&
                      !r.last_exp && !r.occupancy && !r.replay_trace && !r.lat_trace &&
                      !world->succ_off && !r.param_index;
    if (fast) {
      hipLaunchKernelGGL(k_sfma_2_fast, dim3(A.r.n), dim3(64), sfma_lds_bytes(kFastStates), st, A);
      COBEL_HIP_TRY(hipGetLastError());
      return COBEL_OK;
    }
    return launch_sfma<2>(A, (size_t)lds, st);
  }
  if (plain && A.chunk <= 4) {
    A.chunk = 4;
    return launch_sfma<4>(A, (size_t)lds, st);
  }
  if (plain && A.chunk <= 8) {
    A.chunk = 8;
    return launch_sfma<8>(A, (size_t)lds, st);
  }
  // the general kernel: one wave per instance up to 800 experiences, four waves beyond
  // (measured: 14x14 = 784 experiences 9.3e7 vs 7.9e7 reactivations/s in favour of one wave,
  // 20x20 = 1 600 experiences 6.4e6 vs 5.2e7 in favour of four)
  // (COBEL_F_NO_PREFETCH, otherwise unused here, pins the one-wave form for tests)
  if (P.threads == 256) {
    A.chunk = (4 * S + 255) / 256;
    return launch_sfma_wg(A, (size_t)lds, st);
  }
  return launch_sfma<0>(A, (size_t)lds, st);
}
