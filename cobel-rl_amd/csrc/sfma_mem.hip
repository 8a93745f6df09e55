// SFMAMemory on its own — store(), replay() and retrieve_random_batch() as device calls on the
// tables the agent's kernel keeps (cobel_sfma_store, cobel_sfma_replay, cobel_sfma_random_batch).
//
// Store and replay are the agent's: sfma_body (cobel_sfma.h) with MEM = 1 runs its store once per
// instance, with MEM = 2 its replay once per workgroup.  A replay only reads the memory, so the K
// replays of an instance are K workgroups side by side: each has its own inhibition vector and
// priority scratch in LDS and its own place on the memory stream; the strengths and the model come
// from one LDS copy per workgroup (LDS-resident form: 128 B per state, filled from L2 after the
// first workgroup of the instance has touched them) or are read in place (streaming form).
//
// Launch shapes, by cobel_sfma_plan: one wavefront per workgroup up to 800 experiences, four
// beyond, and the streaming form with 4 or 16 wavefronts where the tables do not fit the LDS — the
// general path of the body in every case (all switches of the memory).
//
// Reference behaviour restated (paths relative to /root/reference/src/cobel):
//   memory/sfma.py:195-236 (store), :238-347 (replay), :374-416 (retrieve_random_batch)
#include <cstring>

#include "cobel_sfma.h"

using namespace cobel_sfma;

namespace {

template <int NW, bool BIG, int MEM>
__global__ __launch_bounds__(64 * NW) void k_sfma_mem(const sfma_args A, const sfma_mem_args M) {
  sfma_body<0, NW, false, BIG, MEM>(A, M);
}

template <int NW, bool BIG, int MEM>
int launch_mem(const sfma_args& A, const sfma_mem_args& M, int blocks, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024)
    COBEL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sfma_mem<NW, BIG, MEM>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_sfma_mem<NW, BIG, MEM>), dim3(blocks), dim3(64 * NW), lds, st, A, M);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

struct mem_plan {
  int form, lds, threads;
  uint32_t big_lds;
};

// The form, the LDS and the tier are the agent's plan; the streaming form runs with 4 or 16 waves.
int mem_plan_of(int32_t S, uint32_t flags, mem_plan* P) {
  int32_t out[4];
  if (int rc = cobel_sfma_plan(S, flags, out)) return rc;
  P->form = out[0];
  P->lds = out[1];
  P->threads = out[2];
  P->big_lds = 0;
  if (P->form == 1) {
    if (P->threads != 256) P->threads = 1024;
    // (the tier whose size the plan reports, in the order the plan tries them)
    uint32_t what = kBigNsInLds | kBigRowsInLds;
    if (sfma_big_lds_bytes(S, what) != (size_t)P->lds) what = kBigRowsInLds;
    if (sfma_big_lds_bytes(S, what) != (size_t)P->lds) what = 0;
    COBEL_REQUIRE(sfma_big_lds_bytes(S, what) == (size_t)P->lds, COBEL_E_UNSUPPORTED,
                  "cobel_sfma_mem_plan: no streaming tier of %d B for %d states", P->lds, S);
    P->big_lds = what;
  }
  return COBEL_OK;
}

int check_mem(const cobel_sfma_mem_t* mem, const char* who) {
  COBEL_REQUIRE(mem, COBEL_E_ARG, "%s: NULL mem", who);
  const cobel_sfma_mem_t& m = *mem;
  COBEL_REQUIRE(m.model && m.strength && m.stamp && m.sfma_inst && m.metric && m.counter,
                COBEL_E_ARG,
                "%s: model, strength, stamp, sfma_inst, metric and counter are required", who);
  COBEL_REQUIRE(((uintptr_t)m.strength & 15u) == 0 && ((uintptr_t)m.stamp & 15u) == 0 &&
                    ((uintptr_t)m.model & 7u) == 0 && ((uintptr_t)m.sfma_inst & 7u) == 0,
                COBEL_E_ARG, "%s: strength and stamp must be 16-byte, model and sfma_inst 8-byte aligned",
                who);
  COBEL_REQUIRE(m.n >= 0 && m.n_worlds >= 1, COBEL_E_RANGE, "%s: n = %d, n_worlds = %d", who, m.n,
                m.n_worlds);
  COBEL_REQUIRE(!(m.sfma_flags & COBEL_SF_RECENCY) || (m.recency_tab && m.recency_len > 0),
                COBEL_E_ARG, "%s: recency needs recency_tab", who);
  return sfma_check_sets(m.param_sets, m.param_index, m.n_param_sets, who);
}

// the body's arguments from the memory's: no world, no agent, no monitors
int fill_args(const cobel_sfma_mem_t& m, const mem_plan& P, sfma_args* out) {
  sfma_args& A = *out;
  memset(&A, 0, sizeof(A));
  const int S = m.n_states;
  A.S = S;
  A.n_worlds = m.n_worlds;
  A.r.model = m.model;
  A.r.strength = m.strength;
  A.r.stamp = m.stamp;
  A.r.sfma_inst = m.sfma_inst;
  A.r.metric = m.metric;
  A.r.recency_tab = m.recency_tab;
  A.r.recency_len = m.recency_len;
  A.r.n = m.n;
  A.r.instance_base = m.instance_base;
  A.r.sfma_flags = m.sfma_flags;
  A.r.model_lr = m.model_lr;
  A.r.decay_inhibition = m.decay_inhibition;
  A.r.decay_strength = m.decay_strength;
  A.r.c_step = m.c_step;
  A.r.i_step = m.i_step;
  A.r.r_threshold = m.r_threshold;
  A.r.beta = m.beta;
  A.r.reward_modulation = m.reward_modulation;
  A.r.blend = m.blend;
  A.r.interp_fwd = m.interp_fwd;
  A.r.interp_rev = m.interp_rev;
  A.r.seed = m.seed;
  A.r.param_sets = m.param_sets;
  A.r.param_index = m.param_index;
  A.r.n_param_sets = m.n_param_sets;
  A.model_lr_f = (float)m.model_lr;
  A.big_lds = P.big_lds;
  if (P.form == 1) A.chunk = ((4 * S + P.threads - 1) / P.threads + 3) & ~3;
  else A.chunk = (4 * S + P.threads - 1) / P.threads;
  return COBEL_OK;
}

template <int MEM>
int launch_by_plan(const sfma_args& A, const sfma_mem_args& M, const mem_plan& P, int blocks,
                   hipStream_t st) {
  if (P.form == 1) {
    if (P.threads == 256) return launch_mem<4, true, MEM>(A, M, blocks, (size_t)P.lds, st);
    return launch_mem<16, true, MEM>(A, M, blocks, (size_t)P.lds, st);
  }
  if (P.threads == 256) return launch_mem<4, false, MEM>(A, M, blocks, (size_t)P.lds, st);
  return launch_mem<1, false, MEM>(A, M, blocks, (size_t)P.lds, st);
}

__global__ void k_counter_add(uint32_t* counter, int n, uint32_t by) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) counter[i] += by;
}

// retrieve_random_batch: thread (i, b) counts the entries of the CDF that its uniform has passed
// (searchsorted, side = 'right') and reports the model's record of that experience
__global__ void k_random_batch(const cobel_sfma_mem_t m, int B, const double* cdf,
                               cobel_sfma_event_t* events) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= m.n * B) return;
  const int i = e / B, b = e - i * B;
  const int S = m.n_states, n4 = 4 * S;
  const uint32_t g = m.instance_base + (uint32_t)i;
  const double u = cobel_draw_u01(m.counter[i], COBEL_SUB_DOUBLE + (uint32_t)b, g,
                                  COBEL_STREAM_MEMORY, m.seed);
  int lo = 0, hi = n4;   // first entry > u
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid + 1;
    else hi = mid;
  }
  const int idx = lo < n4 ? lo : n4 - 1;
  const int a = idx / S, s = idx - a * S;   // unravel_index(order='F')
  const uint64_t rec = m.model[(size_t)i * n4 + (size_t)s * 4 + a];
  cobel_sfma_event_t ev;
  ev.sa = (uint32_t)s | ((uint32_t)a << 16) | ((uint32_t)((rec >> 48) & 1u) << 24);
  ev.next = (uint32_t)((rec >> 32) & 0x7fffu);
  ev.reward = __builtin_bit_cast(float, (uint32_t)rec);
  ev.trial = 0;
  ev.td = __builtin_nan("");
  events[e] = ev;
}

}  // namespace

extern "C" int cobel_sfma_mem_plan(int32_t n_states, uint32_t flags, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_sfma_mem_plan: NULL out");
  mem_plan P;
  if (int rc = mem_plan_of(n_states, flags, &P)) return rc;
  out[0] = P.form;
  out[1] = P.lds;
  out[2] = P.threads;
  out[3] = (int32_t)P.big_lds;
  return COBEL_OK;
}

extern "C" int cobel_sfma_store(const cobel_sfma_mem_t* mem, const cobel_sfma_exp_t* experiences,
                                void* stream) {
  if (int rc = check_mem(mem, "cobel_sfma_store")) return rc;
  COBEL_REQUIRE(experiences && ((uintptr_t)experiences & 7u) == 0, COBEL_E_ARG,
                "cobel_sfma_store: experiences must be given, 8-byte aligned");
  mem_plan P;
  if (int rc = mem_plan_of(mem->n_states, mem->flags, &P)) return rc;
  if (mem->n == 0) return COBEL_OK;
  sfma_args A;
  fill_args(*mem, P, &A);
  sfma_mem_args M;
  memset(&M, 0, sizeof(M));
  M.exps = experiences;
  M.counter = mem->counter;
  M.n_replays = 1;
  M.mem_flags = mem->mem_flags;
  return launch_by_plan<1>(A, M, P, mem->n, (hipStream_t)stream);
}

extern "C" int cobel_sfma_replay(const cobel_sfma_mem_t* mem, int32_t n_replays,
                                 int32_t replay_length, const int32_t* start_state,
                                 const int32_t* start_action, cobel_sfma_event_t* events,
                                 int32_t* lengths, double* inhibition, void* stream) {
  if (int rc = check_mem(mem, "cobel_sfma_replay")) return rc;
  COBEL_REQUIRE(n_replays >= 1 && replay_length >= 0, COBEL_E_RANGE,
                "cobel_sfma_replay: n_replays = %d, replay_length = %d", n_replays, replay_length);
  COBEL_REQUIRE(n_replays == 1 || (mem->mem_flags & COBEL_SFM_STRIDED), COBEL_E_ARG,
                "cobel_sfma_replay: %d replays side by side need COBEL_SFM_STRIDED", n_replays);
  COBEL_REQUIRE(lengths && (events || replay_length == 0) && ((uintptr_t)events & 7u) == 0,
                COBEL_E_ARG, "cobel_sfma_replay: events (8-byte aligned) and lengths are required");
  COBEL_REQUIRE((long long)mem->n * n_replays <= 0x7fffffffLL, COBEL_E_RANGE,
                "cobel_sfma_replay: %d x %d replays", mem->n, n_replays);
  mem_plan P;
  if (int rc = mem_plan_of(mem->n_states, mem->flags, &P)) return rc;
  if (mem->n == 0) return COBEL_OK;
  sfma_args A;
  fill_args(*mem, P, &A);
  A.r.batch = replay_length;
  A.r.replay_trace = events;
  A.r.trace_cap = replay_length;
  sfma_mem_args M;
  memset(&M, 0, sizeof(M));
  M.counter = mem->counter;
  M.start_state = start_state;
  M.start_action = start_action;
  M.lengths = lengths;
  M.inhibition = inhibition;
  M.n_replays = n_replays;
  M.mem_flags = mem->mem_flags;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_by_plan<2>(A, M, P, mem->n * n_replays, st)) return rc;
  if (mem->mem_flags & COBEL_SFM_STRIDED) {
    hipLaunchKernelGGL(k_counter_add, dim3((mem->n + 255) / 256), dim3(256), 0, st, mem->counter,
                       mem->n, (uint32_t)n_replays * (uint32_t)(replay_length + 2));
    COBEL_HIP_TRY(hipGetLastError());
  }
  return COBEL_OK;
}

extern "C" int cobel_sfma_random_batch(const cobel_sfma_mem_t* mem, int32_t n_experiences,
                                       const double* random_cdf, cobel_sfma_event_t* events,
                                       void* stream) {
  if (int rc = check_mem(mem, "cobel_sfma_random_batch")) return rc;
  COBEL_REQUIRE(n_experiences >= 0 && (long long)mem->n * n_experiences <= 0x7fffffffLL,
                COBEL_E_RANGE, "cobel_sfma_random_batch: %d experiences", n_experiences);
  COBEL_REQUIRE(random_cdf && (events || n_experiences == 0) && ((uintptr_t)events & 7u) == 0,
                COBEL_E_ARG, "cobel_sfma_random_batch: random_cdf and events are required");
  COBEL_REQUIRE(mem->n_states >= 1 && mem->n_states <= 16383, COBEL_E_RANGE,
                "cobel_sfma_random_batch: %d states", mem->n_states);
  if (mem->n == 0) return COBEL_OK;
  hipStream_t st = (hipStream_t)stream;
  const int total = mem->n * n_experiences;
  if (total > 0) {
    hipLaunchKernelGGL(k_random_batch, dim3((total + 255) / 256), dim3(256), 0, st, *mem,
                       n_experiences, random_cdf, events);
    COBEL_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_counter_add, dim3((mem->n + 255) / 256), dim3(256), 0, st, mem->counter,
                     mem->n, 1u);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
