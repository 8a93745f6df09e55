// Internal declarations shared by the translation units of libcobel_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cobel_hip.h"
#include "cobel_rng.h"

// World record, one per state, 16 B so that a single dwordx4 load returns everything the
// loop needs about a state: where each action leads, and what entering the state pays.
struct __attribute__((aligned(16))) cobel_wrec {
  uint16_t next[4];
  float reward;
  uint32_t terminal;  // 0 / 1
};
static_assert(sizeof(cobel_wrec) == 16, "world record must be 16 bytes");

// The rewarded states of one world (reward != 0), at most 32 of them, and the order in which
// NumPy's pairwise summation (numpy/core/src/umath/loops_utils.h) adds the products of a row with a
// vector that is zero everywhere else: a sum over S elements of which all but k are zero is the sum
// of those k in the grouping the summation tree gives them (an addition of zero changes nothing),
// so k - 1 additions in this order return np.sum(row * R) bit for bit (up to the sign of a zero).
struct cobel_rw_info {
  uint16_t pos[32];     // ascending states
  uint8_t k;            // how many (0 .. 32); 255: more
  uint8_t root;         // slot that holds the sum after the last step
  uint8_t dst[31], src[31];   // step t: value[dst[t]] += value[src[t]]
};
static_assert(sizeof(cobel_rw_info) == 128, "cobel_rw_info layout");

struct cobel_world {
  int32_t n_states, n_worlds, device;
  cobel_wrec* rec;       // [dev] [n_worlds][S]
  uint16_t* starts;      // [dev] concatenated
  int32_t* start_off;    // [dev] [n_worlds + 1]
  int32_t* h_start_off;  // [host] copy for argument checks
  int32_t max_rewarded_states;  // max over worlds of #{s : reward[s] != 0}
  uint32_t* queue;       // [dev] 256 B: ticket counters of the persistent-workgroup kernel for calls
                         // that bring no scratch area (cobel_tab_run_t.scratch)
  cobel_rw_info* rw;     // [dev] [n_worlds] rewarded states + pairwise combine order (four-action worlds)
  // action counts other than four (cobel_world_create_n): `rec` is NULL and these hold the world
  int32_t n_actions;
  uint16_t* next_n;     // [dev] [n_worlds][S][n_actions]
  float* reward_s;      // [dev] [n_worlds][S]
  uint8_t* terminal_s;  // [dev] [n_worlds][S]
  // transition rows that are distributions (cobel_world_set_transitions), else NULL: successors
  // of pair p = (world * S + s) * n_actions + a are succ_state[succ_off[p] .. succ_off[p + 1]) with
  // the normalised cumulative probabilities succ_cdf (last entry of a row = 1)
  uint32_t* succ_off;   // [dev] [n_worlds * S * n_actions + 1]
  uint16_t* succ_state; // [dev] [nnz]
  double* succ_cdf;     // [dev] [nnz]
  int64_t succ_cap;     // entries succ_state / succ_cdf have room for
  // cobel_world_update*: pinned staging, outgrown buffers (world.hip); NULL until the first update
  struct cobel_world_live* live;
};

// the successor Generator.choice(arange(S), p=row) returns for the uniform u (interface/
// gridworld.py:119-123): first entry whose cumulative probability exceeds u
__device__ __forceinline__ int cobel_draw_successor(const uint32_t* __restrict__ off,
                                                    const uint16_t* __restrict__ succ,
                                                    const double* __restrict__ cdf, size_t pair,
                                                    double u) {
  const uint32_t lo = off[pair], hi = off[pair + 1];
  uint32_t k = lo;
  while (k + 1u < hi && !(cdf[k] > u)) ++k;
  return (int)succ[k];
}

// What the routing of a tabular run decides (tab_plan, tabular.hip): which kernel serves it, the
// three numbers cobel_tab_describe reports beside it, and the choices the launchers would otherwise
// work out again.  Filled once per call; the launchers take it as it is.
struct cobel_tab_plan {
  int32_t kind;          // COBEL_TAB_KERNEL_*; 0 with inst_per_wg == 0: nothing to launch (n == 0)
  size_t lds;            // dynamic LDS per workgroup, lds_pad included
  int32_t wg_per_cu;     // workgroups per CU by LDS (lds_workgroups_per_cu; 1 for PWG, 0 for general)
  int32_t inst_per_wg;   // instances per workgroup
  bool replay;           // the run replays: learning, batch > 0, a model or an experience log
  bool occ, wlds;        // wavefront forms: visit counters / the world's records in LDS
  bool fast, midx;       // ... plain Dyna-Q training / with the model digest in HBM
  size_t lds_pad;        // ... COBEL_DEBUG_LDS_PAD (occupancy experiments)
  int lpw;               // lane per instance: instances per wave (64, 32 or 16)
  int nl, ng;            // PWG: waves with Q in LDS / in global memory
  int wpg;               // WQN: waves (= instances) per workgroup
  int lpb;               // general: lanes per workgroup
};

// LDS is handed out in blocks of 1 280 bytes, 128 per CU — not in KiB (measured on MI355X with
// scripts/experiments/exp_occupancy.py: the launch time of k_tab_wpi steps down at 15 360 and at 14 080 bytes
// per workgroup and is flat in between; 16 384 B, a 32 x 32 world, are 13 blocks: nine per CU —
// k_tab_pwg's ONE workgroup per CU takes all 128 blocks for ten).
inline int lds_workgroups_per_cu(size_t bytes) {
  const size_t blocks = (bytes + 1279) / 1280;
  return blocks ? (int)(128 / blocks) : 128;
}

// The kernel files of the tabular agents.  Each `..._plan` knows the limits of its own kernel: it
// returns false where the kernel does not serve the run, else fills its part of the plan.  The
// arguments have passed tab_plan's checks.  Each `..._launch` takes the plan and launches.
// general.hip: any action count / batch size / state count (one lane per instance)
int cobel_env_step_general(const cobel_world* world, int32_t* state, const uint8_t* action,
                           float* reward_out, uint8_t* done_out, uint32_t* env_ctr, uint64_t seed,
                           int32_t n, uint32_t instance_base, hipStream_t st);
void cobel_tab_general_plan(const cobel_tab_run_t& r, cobel_tab_plan& plan);   // (takes every run)
int cobel_tab_general_launch(const cobel_world* world, const cobel_tab_run_t& r,
                             const cobel_tab_plan& plan, hipStream_t st);
// tabular_pwg.hip: plain Dyna-Q training as one persistent workgroup per CU
bool cobel_tab_pwg_plan(const cobel_world* world, const cobel_tab_run_t& r, cobel_tab_plan& plan);
int cobel_tab_pwg_launch(const cobel_world* world, const cobel_tab_run_t& r,
                         const cobel_tab_plan& plan, hipStream_t st);
// tabular_nact.hip: Q-learning on worlds of 1..32 (not four) actions, one wavefront per instance
bool cobel_tab_nact_plan(const cobel_world* world, const cobel_tab_run_t& r, cobel_tab_plan& plan);
int cobel_tab_nact_launch(const cobel_world* world, const cobel_tab_run_t& r,
                          const cobel_tab_plan& plan, hipStream_t st);

// world.hip: the additions NumPy's pairwise sum performs on k non-zero elements at `pos` (ascending)
// of a vector of n elements; returns the slot holding the result (-1: k == 0)
int cobel_pairwise_schedule(int n, const int* pos, int k, uint8_t* dst, uint8_t* src);

// sr_wave.hip: the sparse-reward form of the SR agent (one wavefront per instance)
bool cobel_sr_wave_covers(const cobel_world* world, const cobel_sr_run_t& r);
int cobel_sr_wave_launch(const cobel_world* world, const cobel_sr_run_t& r, hipStream_t st);

int cobel_fail(int code, const char* fmt, ...);
int cobel_device_limits(int device, int* n_cu, size_t* lds_per_cu);   // world.hip (cached per device)
// COBEL_DEBUG_LDS_PAD=<bytes> (occupancy experiments, scripts/experiments/exp_occ*.py): extra dynamic LDS per
// workgroup.  Honoured only if it is a plain number that keeps `base + pad` within `limit`; anything
// else (a stray or malformed variable) is ignored, so it can change occupancy, never break a launch.
size_t cobel_debug_lds_pad(size_t base, size_t limit);
// getenv(name) under the master switch COBEL_DEBUG=1, else NULL (world.hip)
const char* cobel_debug_env(const char* name);
// mlp.hip: the parameter-staging DQN replay kernel (cobel_dqn_replay, mlp_fit.hip, dispatches)
size_t cobel_dqn_replay_lds_bytes(int32_t n_inputs, int32_t is_float64);
int cobel_dqn_replay_lds_launch(const cobel_dqn_replay_t& r, hipStream_t st,
                                unsigned long long* trace /* experiments, or NULL */);
// pma_sr.hip: PMAMemory.update_sr by the blocked kernels on the SR blocks in global memory (any S;
// cobel_pma_update_sr, pma.hip, dispatches), and the LDS of their largest workgroup
// cobel_pma_mem_t as the PMA kernels take it: with the parameter sets of a cobel_pma_mem_sets_t
// behind it (the caller's tail under COBEL_PMA_SETS, zeros otherwise)
struct cobel_pma_mem_x : cobel_pma_mem_t {
  const cobel_pma_param_set_t* param_sets;
  const uint16_t* param_index;
  int32_t n_param_sets, reserved2_;
};
inline cobel_pma_mem_x cobel_pma_expand(const cobel_pma_mem_t* mem) {
  cobel_pma_mem_x x;
  static_cast<cobel_pma_mem_t&>(x) = *mem;
  x.param_sets = nullptr;
  x.param_index = nullptr;
  x.n_param_sets = x.reserved2_ = 0;
  if (mem->flags & COBEL_PMA_SETS) {
    const cobel_pma_mem_sets_t* const t = reinterpret_cast<const cobel_pma_mem_sets_t*>(mem);
    x.param_sets = t->param_sets;
    x.param_index = t->param_index;
    x.n_param_sets = t->n_param_sets;
  }
  return x;
}
// the head of an entry point that was handed `mem_in`: the NULL refusal, then `mem`, the expanded copy
#define COBEL_PMA_MEM(who)                                         \
  COBEL_REQUIRE(mem_in, COBEL_E_ARG, "%s: NULL mem", who);          \
  const cobel_pma_mem_x mem_x_ = cobel_pma_expand(mem_in);         \
  const cobel_pma_mem_x* const mem = &mem_x_
int cobel_pma_sr_blocked(const cobel_pma_mem_x& m, hipStream_t st);
size_t cobel_pma_sr_blocked_lds();
int cobel_world_check(const cobel_world* w, const char* who);   // non-NULL, on the current device
int cobel_world_check4(const cobel_world* w, const char* who);  // ... and a four-action world

#define COBEL_HIP_TRY(expr)                                                                  \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return cobel_fail(COBEL_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                 \
  } while (0)

#define COBEL_REQUIRE(cond, code, ...) \
  do {                                 \
    if (!(cond)) return cobel_fail(code, __VA_ARGS__); \
  } while (0)

// Launches `kernel`; more than 64 KiB of dynamic LDS have to be allowed to the kernel first.
template <typename ARGS>
hipError_t cobel_launch(void (*kernel)(ARGS), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                        const ARGS& args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args);
  return hipGetLastError();
}

// Packed 8-byte records.
//   model entry  : lo = f32 reward estimate, hi = next_state | nonterminal << 16
__host__ __device__ __forceinline__ uint64_t cobel_model_pack(float r, uint32_t ns, uint32_t nt) {
  return (uint64_t)__builtin_bit_cast(uint32_t, r) | ((uint64_t)(ns | (nt << 16)) << 32);
}
//   replay entry (QAgent experience log, worlds of A actions): lo = f32 reward, hi =
//     A <= 4      : state | next_state << 14 | action << 28 | nonterminal << 30  (16 384 states)
//     A = 5 .. 8  : state | next_state << 14 | action << 28 | nonterminal << 31  (16 384 states)
//     A = 9 .. 32 : state | next_state << 13 | action << 26 | nonterminal << 31  ( 8 192 states)
//   (worlds whose states or actions do not fit keep two words per entry: general.hip)
// A is a compile-time constant, or at least known to the compiler to lie on one side of 8 (e.g.
// min(A, 8)), wherever the layout should fold to constant shifts.
__host__ __device__ __forceinline__ uint64_t cobel_log_pack(float r, uint32_t s, uint32_t a,
                                                            uint32_t ns, uint32_t nt, int A) {
  const uint32_t hi = A <= 8 ? (s | (ns << 14) | (a << 28) | (nt << (A <= 4 ? 30 : 31)))
                             : (s | (ns << 13) | (a << 26) | (nt << 31));
  return (uint64_t)__builtin_bit_cast(uint32_t, r) | ((uint64_t)hi << 32);
}
struct cobel_log_rec {
  uint32_t s, a, ns, nt;
  float r;
};
__host__ __device__ __forceinline__ cobel_log_rec cobel_log_unpack(uint64_t rec, int A) {
  const uint32_t hi = (uint32_t)(rec >> 32);
  const float r = __builtin_bit_cast(float, (uint32_t)rec);
  if (A <= 8)
    return {hi & 0x3fffu, (hi >> 28) & (A <= 4 ? 3u : 7u), (hi >> 14) & 0x3fffu,
            (hi >> (A <= 4 ? 30 : 31)) & 1u, r};
  return {hi & 0x1fffu, (hi >> 26) & 31u, (hi >> 13) & 0x1fffu, hi >> 31, r};
}

// Device-side view of the epsilon-greedy CDF table (cobel_policy_table), passed by value.
struct cobel_cdf_table {
  double cdf[16][16][4];
};

#if defined(__HIPCC__)
// ---- wavefront helpers ------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rl(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ float rlf(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ uint32_t rfl(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ float rflf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ uint32_t fbits(float x) { return __builtin_bit_cast(uint32_t, x); }
// successor a of a four-action world record: next[0..3] packed as two words of two u16
__device__ __forceinline__ uint32_t next_of(uint32_t w0, uint32_t w1, int a) {
  const uint32_t w = (a & 2) ? w1 : w0;
  return (a & 1) ? (w >> 16) : (w & 0xffffu);
}
// max of a Q row in two instructions (fmaxf() costs two more: it first quiets each operand)
__device__ __forceinline__ float max4(const float4 v) {
  float m;
  asm("v_max_f32 %0, %1, %2\n\tv_max3_f32 %0, %0, %3, %4"
      : "=&v"(m)
      : "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
  return m;
}
// Orders this wave's LDS traffic across lanes: a memory fence for the compiler, no instruction
// (fences at wavefront scope emit none on gfx950; __builtin_amdgcn_wave_barrier alone does not
// order memory accesses).  Enough only where the LDS is the wave's own or one wave per workgroup
// touches it — no s_barrier.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Per-trial monitors are striped: workgroup b adds into copy b % mon_stripes of each array, so
// that the atomics of thousands of workgroups finishing the same trial indices do not all queue on
// the same few cache lines of one L2 channel (measured on C2: 600 000 atomics per launch onto ~150
// hot addresses cost 1.1 ms of a 2.8 ms launch; Dyna-Q on 65 536 5x5 worlds ran 2x slower).  The
// caller sums the copies.
__device__ __forceinline__ size_t cobel_mon_offset(int32_t mon_stripes, int32_t trial_cap) {
  const unsigned stripes = mon_stripes > 1 ? (unsigned)mon_stripes : 1u;
  return (size_t)((unsigned)blockIdx.x % stripes) * (size_t)trial_cap;
}
#endif
