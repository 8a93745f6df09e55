// Dyna-Q between sessions: DynaQ.replay(), DynaQ.update_q() and DynaQMemory.store() as device calls
// on the tables cobel_tab_run keeps — planning batches with no environment step in between.
//
// k_tab_replay runs n_batches planning batches of B updates per instance.  A batch is what the
// fused kernels plan after a step: B flat indices over all S x 4 pairs in ONE vector draw of the
// memory stream (draw number = the instance's memory counter, element j from sub-stream j), the
// packed model records found there, the updates applied in the reference's order in the planning
// arithmetic (float64 TD, one rounding into the float32 Q), the counter advanced by one.
//   wave form: one wavefront per instance, Q in LDS for the whole call, the updates through the
//     tag rounds of cobel_tab_batch.h, passes of COBEL_MAX_BATCH lanes for larger batches.  The
//     stream is counter based and planning never writes the model, so the records of the next pass
//     are requested before the current one settles.  Several instances share a workgroup where
//     LDS allows; every wave works on its own slice of it and no workgroup barrier exists.
//   lane form: one lane per instance, Q where the caller keeps it, every update in sequence in
//     plain C++: worlds whose Q table exceeds the LDS, and COBEL_F_REPLAY_LANE.
// Both forms leave the same bits.
//
// Reference behaviour restated (paths relative to the reference's src/cobel):
//   agent/dyna_q.py:319-330 (replay), :275-301 (update_q), :290-299 (TD)
//   memory/dyna_q.py:77-96 (store), :122-157 (retrieve_batch)
#include "cobel_common.h"
#include "cobel_tab_batch.h"

namespace {

constexpr int kPassLanes = COBEL_MAX_BATCH;   // planning updates one wavefront takes per pass
constexpr int kLdsLimit = 160 * 1024;
constexpr int kMaxWaves = 8;                  // instances (= wavefronts) per workgroup, at most

struct replay_args {
  cobel_tab_run_t r;
  int32_t S, n_batches, wpg;
};

// hyper-parameters of instance i: launch-wide, or its parameter set — read as the fused kernels do
struct replay_hyper {
  double alpha, gamma;
  float alpha_f, gamma_f;
};
__device__ __forceinline__ replay_hyper hyper_of(const cobel_tab_run_t& r, int i) {
  replay_hyper h = {r.alpha, r.gamma, (float)r.alpha, (float)r.gamma};
  if (r.param_index) {
    const int k = (int)r.param_index[i];
    const cobel_param_set_t* const P = r.param_sets + (k < r.n_param_sets ? k : r.n_param_sets - 1);
    h.alpha = P->alpha;
    h.gamma = P->gamma;
    h.alpha_f = P->alpha_f;
    h.gamma_f = P->gamma_f;
  }
  return h;
}

// planning TD in float64, one rounding on store (NumPy promotion of the reference's expression with a
// float32 table: the sampled `terminal` is np.int64) — the expression of the fused kernels' batch
__device__ __forceinline__ float td_planning(const replay_hyper& h, float r, uint32_t nt, float q,
                                             float m, double* td_out = nullptr) {
  const double gnt = h.gamma * (double)nt;
  double td = (double)r + gnt * (double)m;
  td = td - (double)q;
  if (td_out) *td_out = td;
  return (float)((double)q + h.alpha * td);
}
// online TD in float32 (agent/dyna_q.py:290-299 with Python scalars): the fused kernels' step
__device__ __forceinline__ float td_online(const replay_hyper& h, float r, uint32_t nt, float q,
                                           float m, double* td_out = nullptr) {
  const float gnt = nt ? h.gamma_f : 0.0f;
  float td = r + gnt * m;
  td = td - q;
  if (td_out) *td_out = (double)td;
  return q + h.alpha_f * td;
}

__global__ __launch_bounds__(64 * kMaxWaves) void k_tab_replay(const replay_args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = (int)threadIdx.x & 63;
  // (uniform over the wave: the compiler may keep it in a scalar register)
  const int wave = (int)rfl(threadIdx.x >> 6);
  const int i = (int)blockIdx.x * A.wpg + wave;
  if (i >= A.r.n) return;   // (no workgroup barrier anywhere: a wave may leave on its own)
  const int S = A.S;
  const uint32_t SA = (uint32_t)S * 4u;
  uint32_t* const Qu = reinterpret_cast<uint32_t*>(lds_raw + (size_t)wave * (size_t)S * 16);
  uint4* const Qs = reinterpret_cast<uint4*>(Qu);
  uint4* const Qg = reinterpret_cast<uint4*>(A.r.q) + (size_t)i * S;
  const uint64_t* const model = A.r.model + (size_t)i * SA;
  int32_t* const inst = A.r.inst + (size_t)i * COBEL_I_WORDS;
  const uint32_t g = A.r.instance_base + (uint32_t)i;
  const uint64_t seed = A.r.seed;
  const replay_hyper h = hyper_of(A.r, i);
  const int B = A.r.batch;
  const int passes = (B + kPassLanes - 1) / kPassLanes;

  for (int s = lane; s < S; s += 64) Qs[s] = Qg[s];
  wsync();
  const uint32_t cm = (uint32_t)inst[COBEL_I_CTR_MEMORY];

  // pass p of batch k: updates p * kPassLanes .. of the vector draw number cm + k
  cobel_u4 blk = {0, 0, 0, 0};
  uint32_t blk_idx = ~0u;
  bool blk_valid = false;
  auto fetch = [&](int k, int p, uint32_t& idx, uint64_t& rec) {
    const uint32_t c = cm + (uint32_t)k;
    uint32_t x;
    if (passes == 1) {   // one Philox block serves four consecutive batches
      if (!blk_valid || (c >> 2) != blk_idx) {
        blk = cobel_philox(c >> 2, (uint32_t)lane, g, COBEL_STREAM_MEMORY, seed);
        blk_idx = c >> 2;
        blk_valid = true;
      }
      x = cobel_word(blk, c & 3u);
    } else {
      const cobel_u4 b =
          cobel_philox(c >> 2, (uint32_t)(p * kPassLanes + lane), g, COBEL_STREAM_MEMORY, seed);
      x = cobel_word(b, c & 3u);
    }
    idx = 0u;
    rec = 0;
    const int bp = B - p * kPassLanes < kPassLanes ? B - p * kPassLanes : kPassLanes;
    if (lane < bp) {
      idx = cobel_bounded(x, SA);
      rec = model[idx];
    }
  };

  const int units = A.n_batches * passes;
  uint32_t idx = 0u;
  uint64_t rec = 0;
  if (units > 0) fetch(0, 0, idx, rec);
  int k = 0, p = 0;
  for (int u = 0; u < units; ++u) {
    // the records of the next pass go out before this one settles
    int kn = k, pn = p + 1;
    if (pn == passes) {
      pn = 0;
      kn = k + 1;
    }
    uint32_t idx_next = 0u;
    uint64_t rec_next = 0;
    if (u + 1 < units) fetch(kn, pn, idx_next, rec_next);
    const int bp = B - p * kPassLanes < kPassLanes ? B - p * kPassLanes : kPassLanes;
    const uint32_t hi = (uint32_t)(rec >> 32);
    const float r = __builtin_bit_cast(float, (uint32_t)rec);
    const uint32_t nt = (hi >> 16) & 1u;
    // (a record that names a state outside the world — a table edited by hand — must not take the
    //  row read outside this wave's slice)
    const uint32_t ns = min(hi & 0xffffu, (uint32_t)S - 1u);
    cobel_tab_batch<4>(Qu, idx, ns, lane < bp, bp, lane,
                       [&](float q, float m) -> float { return td_planning(h, r, nt, q, m); });
    idx = idx_next;
    rec = rec_next;
    k = kn;
    p = pn;
  }

  wsync();
  for (int s = lane; s < S; s += 64) Qg[s] = Qs[s];
  if (lane == 0) inst[COBEL_I_CTR_MEMORY] = (int32_t)(cm + (uint32_t)A.n_batches);
}

__global__ __launch_bounds__(64) void k_tab_replay_lane(const replay_args A) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= A.r.n) return;
  const int S = A.S;
  const uint32_t SA = (uint32_t)S * 4u;
  float* const Q = A.r.q + (size_t)i * SA;
  const float4* const Q4 = reinterpret_cast<const float4*>(Q);
  const uint64_t* const model = A.r.model + (size_t)i * SA;
  int32_t* const inst = A.r.inst + (size_t)i * COBEL_I_WORDS;
  const uint32_t g = A.r.instance_base + (uint32_t)i;
  const replay_hyper h = hyper_of(A.r, i);
  const uint32_t cm = (uint32_t)inst[COBEL_I_CTR_MEMORY];
  for (int k = 0; k < A.n_batches; ++k) {
    for (int j = 0; j < A.r.batch; ++j) {
      const uint32_t idx = cobel_draw_bounded(cm + (uint32_t)k, (uint32_t)j, g, COBEL_STREAM_MEMORY,
                                              A.r.seed, SA);
      const uint64_t rec = model[idx];
      const uint32_t hi = (uint32_t)(rec >> 32);
      const uint32_t ns = min(hi & 0xffffu, (uint32_t)S - 1u);
      const float m = max4(Q4[ns]);
      Q[idx] = td_planning(h, __builtin_bit_cast(float, (uint32_t)rec), (hi >> 16) & 1u, Q[idx], m);
    }
  }
  inst[COBEL_I_CTR_MEMORY] = (int32_t)(cm + (uint32_t)A.n_batches);
}

// One given experience per instance (agent/dyna_q.py:275-301), one lane per instance.
__global__ __launch_bounds__(64) void k_tab_update(const replay_args A,
                                                   const cobel_tab_exp_t* __restrict__ exps,
                                                   uint32_t form, double* __restrict__ td_out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= A.r.n) return;
  const cobel_tab_exp_t e = exps[i];
  const int S = A.S;
  double td = 0.0;
  // (state < 0: this instance has no experience; one that names a pair outside the tables is
  //  left out as well — the host checks the ranges and raises)
  if (e.state >= 0 && e.state < S && e.action >= 0 && e.action < 4 && e.next_state >= 0 &&
      e.next_state < S) {
    float* const Q = A.r.q + (size_t)i * S * 4;
    const replay_hyper h = hyper_of(A.r, i);
    const float m = max4(reinterpret_cast<const float4*>(Q)[e.next_state]);
    const uint32_t cell = (uint32_t)e.state * 4u + (uint32_t)e.action;
    const uint32_t nt = e.nonterminal ? 1u : 0u;
    const float q = Q[cell];
    Q[cell] = form == COBEL_UPDATE_PLANNING ? td_planning(h, e.reward, nt, q, m, &td)
                                            : td_online(h, e.reward, nt, q, m, &td);
  }
  td_out[i] = td;
}

// DynaQMemory.store for all instances (memory/dyna_q.py:92-96, float32: d = r - R; R + lr * d), the
// digest entry as the fused kernel writes it.
__global__ __launch_bounds__(64) void k_model_store(uint64_t* __restrict__ model,
                                                    uint16_t* __restrict__ model_index, int n, int S,
                                                    const cobel_tab_exp_t* __restrict__ exps,
                                                    float mlr_f) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const cobel_tab_exp_t e = exps[i];
  if (e.state < 0 || e.state >= S || e.action < 0 || e.action >= 4 || e.next_state < 0 ||
      e.next_state >= S)
    return;
  const size_t sa = (size_t)i * S * 4 + (size_t)e.state * 4 + (size_t)e.action;
  const float R = __builtin_bit_cast(float, (uint32_t)model[sa]);
  const float d = e.reward - R;
  const float Rn = R + mlr_f * d;
  const uint32_t nt = e.nonterminal ? 1u : 0u;
  model[sa] = cobel_model_pack(Rn, (uint32_t)e.next_state, nt);
  if (model_index)
    model_index[sa] = (uint16_t)((uint32_t)e.next_state | (nt << 14) |
                                 (__builtin_bit_cast(uint32_t, Rn) ? 0x8000u : 0u));
}

struct replay_plan {
  int32_t form;    // COBEL_REPLAY_WAVE / COBEL_REPLAY_LANE
  size_t lds;      // per workgroup
  int32_t threads; // per workgroup
  int32_t wpg;     // instances per workgroup
};

// the checks the three Dyna-Q calls share
int check_run(const cobel_world_t* world, const cobel_tab_run_t* run, const char* who) {
  COBEL_REQUIRE(world && run, COBEL_E_ARG, "%s: NULL world/run", who);
  if (int rc = cobel_world_check(world, who)) return rc;
  const cobel_tab_run_t& r = *run;
  COBEL_REQUIRE(r.agent == COBEL_AGENT_DYNAQ, COBEL_E_ARG, "%s: run->agent is not COBEL_AGENT_DYNAQ",
                who);
  COBEL_REQUIRE(world->n_actions == 4, COBEL_E_UNSUPPORTED,
                "%s: Dyna-Q model records are laid out for four-action worlds (this one has %d)", who,
                world->n_actions);
  COBEL_REQUIRE(r.q, COBEL_E_ARG, "%s: q is required", who);
  COBEL_REQUIRE(((uintptr_t)r.q & 15u) == 0, COBEL_E_ARG, "%s: q must be 16-byte aligned", who);
  COBEL_REQUIRE(r.n >= 0, COBEL_E_RANGE, "%s: n = %d", who, r.n);
  COBEL_REQUIRE(!r.param_index || (r.param_sets && r.n_param_sets > 0), COBEL_E_ARG,
                "%s: param_index given without parameter sets", who);
  COBEL_REQUIRE(((uintptr_t)r.param_sets & 7u) == 0 && ((uintptr_t)r.param_index & 1u) == 0,
                COBEL_E_ARG, "%s: misaligned parameter sets", who);
  return COBEL_OK;
}

int plan_replay(const cobel_world_t* world, const cobel_tab_run_t* run, int32_t n_batches,
                replay_plan& P) {
  P = replay_plan{};
  if (int rc = check_run(world, run, "cobel_dynaq_replay")) return rc;
  const cobel_tab_run_t& r = *run;
  COBEL_REQUIRE(r.model && r.inst, COBEL_E_ARG, "cobel_dynaq_replay: model and inst are required");
  COBEL_REQUIRE(((uintptr_t)r.model & 7u) == 0 && ((uintptr_t)r.inst & 7u) == 0, COBEL_E_ARG,
                "cobel_dynaq_replay: model and inst must be 8-byte aligned");
  COBEL_REQUIRE(n_batches >= 0, COBEL_E_RANGE, "cobel_dynaq_replay: n_batches = %d", n_batches);
  COBEL_REQUIRE(r.batch >= 1, COBEL_E_RANGE, "cobel_dynaq_replay: batch %d", r.batch);
  const size_t per = (size_t)world->n_states * 16;
  if ((r.flags & COBEL_F_REPLAY_LANE) || per > (size_t)kLdsLimit) {
    P.form = COBEL_REPLAY_LANE;
    P.threads = 64;
    P.wpg = 64;
    return COBEL_OK;
  }
  // Instances per workgroup: as many as let a CU's LDS hold the most instances (ten tables of a
  // 32 x 32 world are two workgroups of five, not one of eight), but no more than it takes to give
  // every CU a workgroup — a small launch spreads over the chip first.
  int n_cu = 0;
  size_t lds_cu = 0;
  if (int rc = cobel_device_limits(world->device, &n_cu, &lds_cu)) return rc;
  const int fit = (int)((size_t)kLdsLimit / per);
  int wpg = 1, best = 0;
  for (int w = 1; w <= kMaxWaves && w <= fit; ++w) {
    const int held = lds_workgroups_per_cu(per * w) * w;
    if (held >= best) {
      best = held;
      wpg = w;
    }
  }
  const int spread = (r.n + n_cu - 1) / (n_cu > 0 ? n_cu : 1);
  if (wpg > spread) wpg = spread > 0 ? spread : 1;
  P.form = COBEL_REPLAY_WAVE;
  P.wpg = wpg;
  P.threads = 64 * wpg;
  P.lds = per * wpg;
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_dynaq_replay_plan(const cobel_world_t* world, const cobel_tab_run_t* run,
                                       int32_t n_batches, int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_dynaq_replay_plan: NULL out");
  out[0] = out[1] = out[2] = out[3] = 0;
  replay_plan P;
  if (int rc = plan_replay(world, run, n_batches, P)) return rc;
  out[0] = P.form;
  out[1] = (int32_t)P.lds;
  out[2] = P.threads;
  out[3] = P.wpg;
  return COBEL_OK;
}

extern "C" int cobel_dynaq_replay(const cobel_world_t* world, const cobel_tab_run_t* run,
                                  int32_t n_batches, void* stream) {
  replay_plan P;
  if (int rc = plan_replay(world, run, n_batches, P)) return rc;
  if (run->n == 0 || n_batches == 0) return COBEL_OK;
  replay_args A;
  A.r = *run;
  A.S = world->n_states;
  A.n_batches = n_batches;
  A.wpg = P.wpg;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((run->n + P.wpg - 1) / P.wpg);
  if (P.form == COBEL_REPLAY_LANE)
    COBEL_HIP_TRY(cobel_launch(k_tab_replay_lane, dim3(grid), dim3(64), 0, st, A));
  else
    COBEL_HIP_TRY(cobel_launch(k_tab_replay, dim3(grid), dim3((unsigned)P.threads), P.lds, st, A));
  return COBEL_OK;
}

extern "C" int cobel_dynaq_update(const cobel_world_t* world, const cobel_tab_run_t* run,
                                  const cobel_tab_exp_t* exps, uint32_t form, double* td,
                                  void* stream) {
  if (int rc = check_run(world, run, "cobel_dynaq_update")) return rc;
  COBEL_REQUIRE(exps && td, COBEL_E_ARG, "cobel_dynaq_update: NULL experiences / td");
  COBEL_REQUIRE(((uintptr_t)exps & 3u) == 0 && ((uintptr_t)td & 7u) == 0, COBEL_E_ARG,
                "cobel_dynaq_update: misaligned experiences / td");
  COBEL_REQUIRE(form == COBEL_UPDATE_ONLINE || form == COBEL_UPDATE_PLANNING, COBEL_E_ARG,
                "cobel_dynaq_update: unknown form %u", form);
  if (run->n == 0) return COBEL_OK;
  replay_args A;
  A.r = *run;
  A.S = world->n_states;
  A.n_batches = 0;
  A.wpg = 64;
  hipLaunchKernelGGL(k_tab_update, dim3((unsigned)((run->n + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, A, exps, form, td);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_model_store(uint64_t* model, uint16_t* model_index, int32_t n,
                                 int32_t n_states, const cobel_tab_exp_t* exps, double model_lr,
                                 void* stream) {
  COBEL_REQUIRE(model && exps, COBEL_E_ARG, "cobel_model_store: NULL model / experiences");
  COBEL_REQUIRE(((uintptr_t)model & 7u) == 0 && ((uintptr_t)model_index & 1u) == 0 &&
                    ((uintptr_t)exps & 3u) == 0,
                COBEL_E_ARG, "cobel_model_store: misaligned argument");
  COBEL_REQUIRE(n >= 0 && n_states > 0 && n_states <= 16384, COBEL_E_RANGE,
                "cobel_model_store: bad sizes");
  if (n == 0) return COBEL_OK;
  hipLaunchKernelGGL(k_model_store, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, model, model_index, (int)n, (int)n_states, exps,
                     (float)model_lr);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
