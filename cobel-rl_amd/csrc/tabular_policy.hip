// QAgent and Dyna-Q on a Gridworld or a Topology with a Softmax, an ExclusiveEpsilonGreedy or a
// RandomDiscrete policy (policy/softmax.py, policy/greedy.py:91-147, policy/random.py:13-75 of the
// reference) — one WAVEFRONT per instance, a kernel and an entry point of their own: runs with an
// EpsilonGreedy policy take cobel_tab_run and its kernels exactly as before.
//
// Layout (the shape of k_tab_wqn, tabular_nact.hip): for the whole call the instance's Q table lives
// in LDS, rows padded to eight floats (pad cells -inf: a row maximum needs no action count), beside
// the world as u16 next[S][8] + {reward, terminal}[S] — one copy per workgroup where all its instances
// share a world — and the allowed actions of every state as one word.  One to eight actions, up to
// 1 024 states, transition tables only.  Dyna-Q's model records and QAgent's log stay in global memory.
//
// Formats and order of effects are k_tab_general's (general.hip): the same q, model, replay_log,
// inst, monitor, last_exp and counter formats, the same Philox streams — the trial start from the env
// stream, ONE draw of the policy stream per selection, element j of a batch from sub-stream j of the
// memory stream —, the env step, the model store and the online TD update in float32, the log append,
// then the batch: Dyna-Q's in float64 rounded once on store, QAgent's in float32, both as the
// speculative rounds of cobel_tab_batch.h.  A session here and a session on the other kernels
// interleave on the same agent.
//
// Selection, in float64 whatever the table dtype (cobel_policy.h), by a GROUP of eight lanes, lane a
// holding value a of the row (in the run kernel the eight groups of the wave hold the same row and
// end with the same bits; cobel_policy_select_n gives every group a row of its own):
//   Softmax      e_a = exp((v_a - max) * beta) over the allowed actions, side by side;
//                sum = ((e_0 + e_1) + e_2) + ... in action order, one chain every lane runs; p_a = e_a / sum
//   Exclusive    ties by exact equality; p_a = ((1 - eps) * tie_a) / n_ties, then
//                p_a += (eps * !tie_a) / max(n_allowed - n_ties, 1) — the reference's operations in its order
//   both         Generator.choice: cum_a = ((p_0 + p_1) + ...) + p_a, action = #{a < A - 1 : cum_a / cum_{A-1} <= u}
//   Random       int(rng.integers(A)): ONE bounded draw (cobel_bounded of the draw's word); values and
//                mask are ignored, as the reference ignores them
// The file is compiled with -ffp-contract=off: every operation rounds.
//
// Why a gather cannot see a stale record.  Lane 0 stores the model record / the log record of a step;
// the lanes of the batch read records of earlier steps.  (1) The record of the current step is never
// read back: it is forwarded from registers.  (2) The old model record of a step is read by lane 0,
// which wrote it.  (3) Every step with a batch waits for its gathered loads (vmcnt(0): on gfx9 the
// counter covers the wavefront's stores too, and they retire in order), so the stores of a step have
// reached the L2 before the gather of the next one is issued; the gathers are relaxed agent-scope
// atomic loads, served by that L2 and not by a line the CU's vector cache kept.
//
// Nothing in here is tuned: every lane evaluates the Philox blocks it needs itself, the selection
// moves its values through ds_bpermute, and a step waits for each of its trips to memory.
#include <math.h>

#include <vector>

#include "cobel_common.h"
#include "cobel_tab_batch.h"
#include "cobel_tab_session.h"

namespace {

constexpr int kW = 8;             // values per row = lanes per selection group
constexpr int kMaxStates = 1024;

// ---- the selection -------------------------------------------------------------------------------
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
  for (int o = 1; o < kW; o <<= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
// the lanes of this lane's group for which `pass` holds (wave-uniform control flow)
__device__ __forceinline__ int group_count(bool pass, int lane) {
  const unsigned long long b = __ballot(pass);
  return __popc((uint32_t)(b >> (lane & ~(kW - 1))) & 0xffu);
}
// Generator.choice(arange(A), p = the group's probabilities) for the uniform u
__device__ __forceinline__ int group_choice(double p, int a, int A, double u, int lane) {
  double run = 0.0, cum = 0.0, total = 0.0;
#pragma unroll
  for (int k = 0; k < kW; ++k) {
    const double pk = __shfl(p, k, kW);
    run = (k == 0) ? pk : run + pk;
    cum = (k == a) ? run : cum;
    total = (k == A - 1) ? run : total;
  }
  return group_count(a < A - 1 && cum / total <= u, lane);
}
// v: the value of action a (this lane's); allowed: bit k set = action k takes part (at least one);
// param: beta / epsilon; u: the uniform draw (Softmax, Exclusive); word: the 32-bit word of the
// bounded draw (Random); p: this lane's probability.  Wave-uniform control flow.
template <int POLICY>
__device__ __forceinline__ int policy_select(double v, int a, int A, uint32_t allowed, double param,
                                             double u, uint32_t word, int lane, double& p) {
  if (POLICY == COBEL_POLICY_RANDOM) {
    p = a < A ? 1.0 / (double)A : 0.0;
    return (int)cobel_bounded(word, (uint32_t)A);
  }
  const bool on = a < A && ((allowed >> a) & 1u);
  const double m = group_max(on ? v : -__builtin_huge_val());
  if (POLICY == COBEL_POLICY_SOFTMAX) {
    const double e = on ? exp((v - m) * param) : 0.0;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kW; ++k) sum = sum + __shfl(e, k, kW);
    p = on ? e / sum : 0.0;
  } else {
    const bool tie = on && v == m;
    const int n_on = group_count(on, lane), n_ties = group_count(tie, lane);
    const double t = tie ? 1.0 : 0.0;
    p = ((1.0 - param) * t) / (double)n_ties;
    p = p + (param * (1.0 - t)) / (double)max(n_on - n_ties, 1);
    p = on ? p : 0.0;
  }
  return group_choice(p, a, A, u, lane);
}

// ---- the run kernel ------------------------------------------------------------------------------
struct pol_args {
  const cobel_wrec* rec;       // four-action worlds
  const uint16_t* next_n;      // other action counts: [W][S][A]
  const float* reward_s;       // [W][S]
  const uint8_t* terminal_s;   // [W][S]
  const uint16_t* starts;
  const int32_t* start_off;
  int32_t S, n_worlds, A;
  int32_t wpg;                 // wavefronts (instances) per workgroup
  int32_t shared_world;        // one world: the workgroup keeps ONE copy of it
  cobel_tab_run_t r;
  const double* policy_params; // [n_param_sets] or NULL
  double policy_param;
  float alpha_f, gamma_f, model_lr_f;
};

__host__ __device__ inline size_t pol_mask_bytes(int S) { return ((size_t)S * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pol_world_bytes(int S) {
  return ((size_t)S * (2 * kW + 8) + 15) & ~(size_t)15;
}
// LDS of a workgroup of `wpg` instances: allowed actions | world(s) | per instance Q
__host__ __device__ inline size_t pol_lds_bytes(int S, int wpg, bool shared) {
  return pol_mask_bytes(S) + pol_world_bytes(S) * (shared ? 1 : wpg) + (size_t)wpg * S * kW * 4;
}

__device__ __forceinline__ uint64_t load_l2(const uint64_t* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

template <int AGENT, int POLICY>
__global__ __launch_bounds__(512) void k_tab_pol(const pol_args G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int S = G.S, A = G.A;
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = (int)rfl(threadIdx.x >> 6);
  const int i = (int)blockIdx.x * G.wpg + wave;
  const bool present = i < G.r.n;
  const uint32_t g = G.r.instance_base + (uint32_t)(present ? i : 0);
  const int world = (int)(g % (uint32_t)G.n_worlds);
  const size_t wbase = (size_t)world * S;

  // ---- LDS carve-up -----------------------------------------------------------------------------
  uint32_t* const maskL = reinterpret_cast<uint32_t*>(lds_raw);          // [S] allowed actions
  size_t off = pol_mask_bytes(S);
  const size_t wbytes = pol_world_bytes(S);
  unsigned char* const wl = lds_raw + off + (G.shared_world ? 0 : (size_t)wave * wbytes);
  off += G.shared_world ? wbytes : wbytes * (size_t)G.wpg;
  uint16_t* const nextL = reinterpret_cast<uint16_t*>(wl);               // [S][8]
  uint2* const RT = reinterpret_cast<uint2*>(wl + (size_t)S * 2 * kW);   // [S] {reward bits, terminal}
  unsigned char* const mine = lds_raw + off + (size_t)wave * ((size_t)S * kW * 4);
  uint32_t* const Qu = reinterpret_cast<uint32_t*>(mine);                // [S][8] (the batch)
  const uint4* const Q4 = reinterpret_cast<const uint4*>(mine);          // [S][2] (row maxima)
  float* const Qf = reinterpret_cast<float*>(mine);

  // ---- allowed actions, the world(s), this instance's Q table ---------------------------------------
  {
    const uint32_t all = (1u << A) - 1u;
    const uint8_t* const amask = (G.r.flags & COBEL_F_MASK_ACTIONS) ? G.r.action_mask : nullptr;
    for (int s = (int)threadIdx.x; s < S; s += (int)blockDim.x)
      maskL[s] = amask ? ((uint32_t)amask[s] & all) : all;
    const int nthr = G.shared_world ? (int)blockDim.x : 64;
    const int tid = G.shared_world ? (int)threadIdx.x : lane;
    if (G.shared_world || present) {
      for (int e = tid; e < S * kW; e += nthr) {
        const int s = e / kW, a = e % kW;
        uint16_t nx = (uint16_t)s;
        if (a < A) nx = G.rec ? G.rec[wbase + s].next[a] : G.next_n[(wbase + s) * A + a];
        nextL[e] = nx < S ? nx : (uint16_t)s;
      }
      for (int s = tid; s < S; s += nthr)
        RT[s] = G.rec ? make_uint2(fbits(G.rec[wbase + s].reward), G.rec[wbase + s].terminal & 1u)
                      : make_uint2(fbits(G.reward_s[wbase + s]), (uint32_t)(G.terminal_s[wbase + s] != 0));
    }
  }
  float* const Qg = G.r.q + (size_t)(present ? i : 0) * S * A;
  if (present) {
    for (int e = lane; e < S * kW; e += 64) {
      const int s = e / kW, a = e % kW;
      Qf[e] = a < A ? Qg[(size_t)s * A + a] : -__builtin_huge_valf();
    }
  }
  __syncthreads();
  if (!present) return;

  // ---- the instance's state ---------------------------------------------------------------------
  int32_t* const inst = G.r.inst + (size_t)i * COBEL_I_WORDS;
  int state = min(max(inst[COBEL_I_STATE], 0), S - 1);
  int step = inst[COBEL_I_STEP];
  int trial = inst[COBEL_I_TRIAL];
  uint32_t ce = (uint32_t)inst[COBEL_I_CTR_ENV];
  uint32_t cp = (uint32_t)inst[COBEL_I_CTR_POLICY];
  uint32_t cm = (uint32_t)inst[COBEL_I_CTR_MEMORY];
  uint32_t loglen = (uint32_t)inst[COBEL_I_LOG_LEN];
  uint32_t iflags = (uint32_t)inst[COBEL_I_FLAGS];
  double trew = *reinterpret_cast<const double*>(inst + COBEL_I_REWARD_LO);
  unsigned long long executed = 0ull, batches = 0ull;

  const uint32_t flags = G.r.flags;
  const bool learn = (flags & COBEL_F_LEARN) != 0;
  const uint32_t pol_stream =
      (flags & COBEL_F_TEST_STREAM) ? COBEL_STREAM_POLICY_TEST : COBEL_STREAM_POLICY;
  const uint64_t seed = G.r.seed;
  const int start_lo = G.start_off[world];
  const uint32_t start_cnt = (uint32_t)(G.start_off[world + 1] - start_lo);
  uint64_t* const model = AGENT == COBEL_AGENT_DYNAQ ? G.r.model + (size_t)i * S * A : nullptr;
  uint16_t* const mindex =
      (AGENT == COBEL_AGENT_DYNAQ && G.r.model_index) ? G.r.model_index + (size_t)i * S * A : nullptr;
  uint64_t* const rlog = (AGENT == COBEL_AGENT_Q && G.r.replay_log)
                             ? G.r.replay_log + (size_t)i * G.r.log_cap : nullptr;
  const uint32_t cap = rlog ? (uint32_t)G.r.log_cap : 0u;
  loglen = min(loglen, cap);
  const int A_log = min(A, 8);
  const int B = (learn && !(flags & COBEL_F_NO_REPLAY) &&
                 (AGENT == COBEL_AGENT_DYNAQ || rlog != nullptr)) ? min(G.r.batch, COBEL_MAX_BATCH) : 0;
  const uint32_t SA = (uint32_t)(S * A);

  // hyper-parameters: launch-wide, or this instance's parameter set and its entry of policy_params
  double alpha = G.r.alpha, gamma = G.r.gamma, pparam = G.policy_param;
  float alpha_f = G.alpha_f, gamma_f = G.gamma_f, mlr_f = G.model_lr_f;
  if (G.r.param_index) {
    const int k = min((int)G.r.param_index[i], G.r.n_param_sets - 1);
    const cobel_param_set_t* const P = G.r.param_sets + k;
    alpha = P->alpha;
    gamma = P->gamma;
    alpha_f = P->alpha_f;
    gamma_f = P->gamma_f;
    mlr_f = P->model_lr_f;
    if (G.policy_params) pparam = G.policy_params[k];
  }

  const size_t mstripe = cobel_mon_offset(G.r.mon_stripes, G.r.trial_cap);
  int budget = G.r.step_budget > 0 ? G.r.step_budget : 0x7fffffff;
  const int k8 = lane & (kW - 1);

  while (true) {
    if (!(iflags & 1u)) {
      if (trial >= G.r.trials_target) break;
      state = min((int)G.starts[start_lo + (int)cobel_draw_bounded(ce, 0u, g, COBEL_STREAM_ENV, seed,
                                                                   start_cnt)], S - 1);
      ce += 1u;
      step = 0;
      trew = 0.0;
      iflags |= 1u;
    }
    if (budget == 0) break;
    budget -= 1;

    // ---- select: one draw of the policy stream ------------------------------------------------------
    const float qc = Qf[(uint32_t)state * kW + (uint32_t)k8];
    int a;
    {
      double u = 0.0, p;
      uint32_t word = 0u;
      if (POLICY == COBEL_POLICY_RANDOM)
        word = cobel_word(cobel_philox(cp >> 2, 0u, g, pol_stream, seed), cp & 3u);
      else
        u = cobel_draw_u01(cp, 0u, g, pol_stream, seed);
      cp += 1u;
      a = (int)rfl((uint32_t)policy_select<POLICY>((double)qc, k8, A, maskL[state], pparam, u, word,
                                                   lane, p));
      a = min(a, A - 1);
    }
    // ---- env.step (interface/gridworld.py:115-126, interface/topology.py:126-157) ---------------------
    const int ns = (int)nextL[(uint32_t)state * kW + (uint32_t)a];
    const uint2 rt = RT[ns];
    const float r = __builtin_bit_cast(float, rt.x);
    const uint32_t end = rt.y, nt = 1u - end;
    const uint32_t sa = (uint32_t)(state * A + a);
    float td_online = 0.0f;
    uint64_t fresh = 0;           // the record this step stored: Dyna-Q's model entry, QAgent's experience
    bool appended = false;
    if (learn) {
      if (AGENT == COBEL_AGENT_DYNAQ) {   // memory/dyna_q.py:92-96, float32; lane 0 owns the records
        uint64_t rec = 0;
        if (lane == 0) {
          const float R = __builtin_bit_cast(float, (uint32_t)model[sa]);
          const float d = r - R;
          const float Rn = R + mlr_f * d;
          rec = cobel_model_pack(Rn, (uint32_t)ns, nt);
          model[sa] = rec;
          if (mindex)
            mindex[sa] = (uint16_t)((uint32_t)ns | (nt << 14) | (fbits(Rn) ? 0x8000u : 0u));
        }
        fresh = ((uint64_t)rfl((uint32_t)(rec >> 32)) << 32) | rfl((uint32_t)rec);
      }
      {   // online TD, float32 (agent/dyna_q.py:290-299, agent/q.py:305-313)
        const float m = cobel_row_max<kW>(Q4 + (uint32_t)ns * (kW / 4));
        const float qsa = Qf[(uint32_t)state * kW + (uint32_t)a];
        const float gnt = nt ? gamma_f : 0.0f;
        float td = r + gnt * m;
        td = td - qsa;
        if (lane == 0) Qf[(uint32_t)state * kW + (uint32_t)a] = qsa + alpha_f * td;
        td_online = td;
      }
      if (AGENT == COBEL_AGENT_Q && rlog) {   // agent/q.py:213 (a full log takes no record)
        fresh = cobel_log_pack(r, (uint32_t)state, (uint32_t)a, (uint32_t)ns, nt, A_log);
        appended = loglen < cap;
        if (appended && lane == 0) rlog[loglen] = fresh;
        if (appended) loglen += 1u;
      }
      wsync();
    }
    if (G.r.last_exp && lane == 0) {
      int32_t* const e = G.r.last_exp + (size_t)i * 6;
      e[0] = state;
      e[1] = a;
      e[2] = ns;
      e[3] = (int32_t)nt;
      e[4] = __builtin_bit_cast(int32_t, r);
      e[5] = __builtin_bit_cast(int32_t, td_online);
    }
    trew += (double)r;
    executed += 1ull;
    if (G.r.occupancy && lane == 0) atomicAdd(G.r.occupancy + wbase + ns, 1ull);
    const bool trial_over = end || (step + 1 >= G.r.steps_per_trial);
    state = ns;

    // ---- the batch: lane j < B holds update j (cobel_tab_batch.h) -------------------------------------
    if (B > 0) {
      const bool on = lane < B;
      if (AGENT == COBEL_AGENT_DYNAQ) {   // memory/dyna_q.py:137-155 + agent/dyna_q.py:327-330
        uint32_t idx = 0u;
        uint64_t rec = 0;
        if (on) {
          idx = cobel_draw_bounded(cm, (uint32_t)lane, g, COBEL_STREAM_MEMORY, seed, SA);
          rec = idx == sa ? fresh : load_l2(model + idx);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t hi = (uint32_t)(rec >> 32);
        const uint32_t ps = idx / (uint32_t)A, pa = idx % (uint32_t)A;
        const uint32_t pns = min(hi & 0xffffu, (uint32_t)(S - 1)), pnt = (hi >> 16) & 1u;
        const double pr = (double)__builtin_bit_cast(float, (uint32_t)rec);
        cobel_tab_batch<kW>(Qu, ps * kW + pa, pns, on, B, lane, [&](float q, float m) -> float {
          const double gnt = gamma * (double)pnt;
          double td = pr + gnt * (double)m;
          td = td - (double)q;
          return (float)((double)q + alpha * td);
        });
        batches += 1ull;
      } else if (loglen > 0u) {           // agent/q.py:344-354: ONE integers(0, len(M), B)
        uint64_t rec = 0;
        if (on) {
          const uint32_t idx = cobel_draw_bounded(cm, (uint32_t)lane, g, COBEL_STREAM_MEMORY, seed, loglen);
          rec = (appended && idx + 1u == loglen) ? fresh : load_l2(rlog + idx);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const cobel_log_rec e = cobel_log_unpack(rec, A_log);
        const uint32_t ps = min(e.s, (uint32_t)(S - 1)), pns = min(e.ns, (uint32_t)(S - 1));
        cobel_tab_batch<kW>(Qu, ps * kW + (e.a & 7u), pns, on, B, lane, [&](float q, float m) -> float {
          const float gnt = e.nt ? gamma_f : 0.0f;
          float td = e.r + gnt * m;
          td = td - q;
          return q + alpha_f * td;
        });
        batches += 1ull;
      }
      cm += 1u;
    }

    if (trial_over) {
      if (lane == 0 && trial >= 0 && trial < G.r.trial_cap) {
        const size_t mo = mstripe + (size_t)trial;
        if (G.r.lat_sum) atomicAdd(G.r.lat_sum + mo, (unsigned long long)step);
        if (G.r.lat_cnt) atomicAdd(G.r.lat_cnt + mo, 1ull);
        if (G.r.reward_sum) atomicAdd(G.r.reward_sum + mo, trew);
        if (G.r.resp_cnt && trew > 0.0) atomicAdd(G.r.resp_cnt + mo, 1ull);
        if (G.r.lat_trace) G.r.lat_trace[(size_t)i * G.r.trial_cap + trial] = step;
      }
      trial += 1;
      iflags &= ~1u;
    } else {
      step += 1;
    }
  }

  // ---- write back -------------------------------------------------------------------------------
  wsync();
  for (int e = lane; e < S * kW; e += 64) {
    const int s = e / kW, a = e % kW;
    if (a < A) Qg[(size_t)s * A + a] = Qf[e];
  }
  if (lane == 0) {
    inst[COBEL_I_STATE] = state;
    inst[COBEL_I_STEP] = step;
    inst[COBEL_I_TRIAL] = trial;
    inst[COBEL_I_CTR_ENV] = (int32_t)ce;
    inst[COBEL_I_CTR_POLICY] = (int32_t)cp;
    inst[COBEL_I_CTR_MEMORY] = (int32_t)cm;
    inst[COBEL_I_LOG_LEN] = (int32_t)loglen;
    inst[COBEL_I_FLAGS] = (int32_t)iflags;
    *reinterpret_cast<double*>(inst + COBEL_I_REWARD_LO) = trew;
    *reinterpret_cast<unsigned long long*>(inst + COBEL_I_STEPS_LO) += executed;
    if (G.r.steps_done && executed) atomicAdd(G.r.steps_done, executed);
    if (G.r.batches_done && batches) atomicAdd(G.r.batches_done, batches);
  }
}

// ---- the single-call form: one group of eight lanes per row ------------------------------------------
template <int POLICY>
__global__ __launch_bounds__(256) void k_policy_select_n(const double* __restrict__ values,
                                                         const uint8_t* __restrict__ mask,
                                                         const double* __restrict__ u,
                                                         const uint64_t* __restrict__ k,
                                                         const double* __restrict__ param, int n_param,
                                                         uint8_t* __restrict__ action_out,
                                                         double* __restrict__ probs_out, int n, int A) {
  const int lane = (int)threadIdx.x & 63;
  const int a = lane & (kW - 1);
  const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / kW;
  const bool valid = r < (long long)n;
  const size_t row = valid ? (size_t)r : 0;
  const bool random = POLICY == COBEL_POLICY_RANDOM;
  const double v = (!random && a < A) ? values[row * A + a] : 0.0;
  const uint32_t all = (1u << A) - 1u;
  uint32_t allowed = (!random && mask) ? ((uint32_t)mask[row] & all) : all;
  if (!allowed) allowed = all;     // (refused on the host; never a division by an empty sum)
  double p;
  const int action = policy_select<POLICY>(v, a, A, allowed, random ? 0.0 : param[n_param > 1 ? row : 0],
                                           random ? 0.0 : u[row], random ? (uint32_t)k[row] : 0u, lane, p);
  if (valid) {
    if (probs_out && a < A) probs_out[row * A + a] = p;
    if (action_out && a == 0) action_out[row] = (uint8_t)action;
  }
}

// ---- argument checks -------------------------------------------------------------------------------
const char* policy_name(int policy) {
  return policy == COBEL_POLICY_SOFTMAX ? "Softmax"
         : policy == COBEL_POLICY_EXCLUSIVE ? "ExclusiveEpsilonGreedy" : "RandomDiscrete";
}

int check_param(int policy, double v, const char* who) {
  if (policy == COBEL_POLICY_SOFTMAX)
    COBEL_REQUIRE(v > 0.0, COBEL_E_ARG, "%s: beta %g is not positive", who, v);
  if (policy == COBEL_POLICY_EXCLUSIVE)
    COBEL_REQUIRE(v >= 0.0 && v <= 1.0, COBEL_E_ARG, "%s: epsilon %g outside [0, 1]", who, v);
  return COBEL_OK;
}

// Everything that can be said without a device, then the device the world lives on.
int check_run(const cobel_world_t* world, const cobel_tab_policy_run_t* run, const char* who) {
  COBEL_REQUIRE(world && run, COBEL_E_ARG, "%s: NULL world/run", who);
  const cobel_tab_run_t& r = run->run;
  // (the table is staged into LDS value by value, epsilon is no parameter of the run)
  if (int rc = cobel_tab_run_check(world, r, who, COBEL_CHECK_TABLES)) return rc;
  COBEL_REQUIRE(((uintptr_t)run->policy_params & 7u) == 0, COBEL_E_ARG,
                "%s: policy_params must be 8-byte aligned", who);
  COBEL_REQUIRE(run->policy == COBEL_POLICY_SOFTMAX || run->policy == COBEL_POLICY_EXCLUSIVE ||
                    run->policy == COBEL_POLICY_RANDOM,
                COBEL_E_ARG, "%s: unknown policy %d (COBEL_POLICY_SOFTMAX, _EXCLUSIVE, _RANDOM)", who,
                run->policy);
  COBEL_REQUIRE(!run->policy_params || r.param_index, COBEL_E_ARG,
                "%s: policy_params given without param_index", who);
  if (!run->policy_params)
    if (int rc = check_param(run->policy, run->policy_param, who)) return rc;
  // what this kernel does not serve
  COBEL_REQUIRE(world->n_actions >= 1 && world->n_actions <= kW, COBEL_E_UNSUPPORTED,
                "%s: %d actions (a %s run serves 1 to %d)", who, world->n_actions,
                policy_name(run->policy), kW);
  COBEL_REQUIRE(!(r.agent == COBEL_AGENT_Q && r.replay_log) ||
                    COBEL_LOG_WORDS(world->n_actions, world->n_states) == 1,
                COBEL_E_UNSUPPORTED, "%s: the experience log of a world of %d states takes two words "
                "per entry (a %s run serves logs of one word: up to 16384 states)", who,
                world->n_states, policy_name(run->policy));
  COBEL_REQUIRE(world->n_states >= 1 && world->n_states <= kMaxStates, COBEL_E_UNSUPPORTED,
                "%s: %d states (a %s run serves 1 to %d)", who, world->n_states,
                policy_name(run->policy), kMaxStates);
  COBEL_REQUIRE(r.batch <= COBEL_MAX_BATCH, COBEL_E_UNSUPPORTED,
                "%s: batch %d (a %s run serves 0 to %d)", who, r.batch, policy_name(run->policy),
                COBEL_MAX_BATCH);
  COBEL_REQUIRE(!(r.flags & COBEL_F_EPISODIC), COBEL_E_UNSUPPORTED,
                "%s: episodic replay (COBEL_F_EPISODIC) is not served with a %s policy", who,
                policy_name(run->policy));
  COBEL_REQUIRE(!world->succ_off, COBEL_E_UNSUPPORTED,
                "%s: the world's transition rows are distributions (cobel_world_set_transitions); "
                "a %s run steps transition tables", who, policy_name(run->policy));
  COBEL_REQUIRE(world->n_actions == 4 || !r.model_index, COBEL_E_ARG,
                "%s: the model digest exists for four-action worlds only", who);
  return cobel_world_check(world, who);
}

// Instances per workgroup (1, 2, 4 or 8; they share the world's copy where there is one world) and the
// LDS they take (cobel_wave_plan).
int plan_run(const cobel_world_t* world, const cobel_tab_run_t& r, int& wpg, size_t& lds, const char* who) {
  const int S = world->n_states;
  const bool shared = world->n_worlds == 1;
  int n_cu = 0;
  size_t lds_cu = 0;
  if (int rc = cobel_device_limits(world->device, &n_cu, &lds_cu)) return rc;
  wpg = cobel_wave_plan(lds_cu, n_cu, r.n, shared,
                        [&](int w) { return pol_lds_bytes(S, w, shared); });
  lds = pol_lds_bytes(S, wpg, shared);
  COBEL_REQUIRE(lds <= lds_cu, COBEL_E_UNSUPPORTED, "%s: %zu bytes of LDS per instance, %zu per CU",
                who, lds, lds_cu);
  return COBEL_OK;
}

// What has to be read back to be checked.
template <typename T>
int fetch(std::vector<T>& host, const T* dev, size_t count, hipStream_t st) {
  host.resize(count);
  COBEL_HIP_TRY(hipMemcpyAsync(host.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
  COBEL_HIP_TRY(hipStreamSynchronize(st));
  return COBEL_OK;
}
// no row of `count` action masks may mask all A actions (`row`: what a row is to the caller)
int check_masks(const uint8_t* mask, int count, int A, const char* row, hipStream_t st,
                const char* who) {
  std::vector<uint8_t> rows;
  if (int rc = fetch(rows, mask, (size_t)count, st)) return rc;
  const uint32_t all = (1u << A) - 1u;
  for (int k = 0; k < count; ++k)
    COBEL_REQUIRE((rows[k] & all) != 0u, COBEL_E_ARG, "%s: the action mask masks all actions of "
                  "%s %d", who, row, k);
  return COBEL_OK;
}
// every policy parameter of the `count` at `param` is in the policy's range
int check_params(int policy, const double* param, int count, hipStream_t st, const char* who) {
  std::vector<double> vals;
  if (int rc = fetch(vals, param, (size_t)count, st)) return rc;
  for (double v : vals)
    if (int rc = check_param(policy, v, who)) return rc;
  return COBEL_OK;
}

template <int AGENT>
auto run_variant(int policy) -> void (*)(const pol_args) {
  if (policy == COBEL_POLICY_SOFTMAX) return &k_tab_pol<AGENT, COBEL_POLICY_SOFTMAX>;
  if (policy == COBEL_POLICY_EXCLUSIVE) return &k_tab_pol<AGENT, COBEL_POLICY_EXCLUSIVE>;
  return &k_tab_pol<AGENT, COBEL_POLICY_RANDOM>;
}

}  // namespace

extern "C" int cobel_tab_policy_plan(const cobel_world_t* world, const cobel_tab_policy_run_t* run,
                                     int32_t* out) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_tab_policy_plan: NULL out");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (int rc = check_run(world, run, "cobel_tab_policy_plan")) return rc;
  if (run->run.n == 0) return COBEL_OK;
  int wpg = 1;
  size_t lds = 0;
  if (int rc = plan_run(world, run->run, wpg, lds, "cobel_tab_policy_plan")) return rc;
  out[0] = (int32_t)lds;
  out[1] = 64 * wpg;
  out[2] = wpg;
  out[3] = (run->run.n + wpg - 1) / wpg;
  return COBEL_OK;
}

extern "C" int cobel_tab_policy_run(const cobel_world_t* world, const cobel_tab_policy_run_t* run,
                                    void* stream) {
  const char* const who = "cobel_tab_policy_run";
  if (int rc = check_run(world, run, who)) return rc;
  const cobel_tab_run_t& r = run->run;
  if (r.n == 0) return COBEL_OK;
  hipStream_t st = (hipStream_t)stream;
  if (run->policy != COBEL_POLICY_RANDOM && (r.flags & COBEL_F_MASK_ACTIONS))
    if (int rc = check_masks(r.action_mask, world->n_states, world->n_actions, "state", st, who))
      return rc;
  if (run->policy_params)
    if (int rc = check_params(run->policy, run->policy_params, r.n_param_sets, st, who)) return rc;
  int wpg = 1;
  size_t lds = 0;
  if (int rc = plan_run(world, r, wpg, lds, who)) return rc;
  pol_args G;
  G.rec = world->rec;
  G.next_n = world->next_n;
  G.reward_s = world->reward_s;
  G.terminal_s = world->terminal_s;
  G.starts = world->starts;
  G.start_off = world->start_off;
  G.S = world->n_states;
  G.n_worlds = world->n_worlds;
  G.A = world->n_actions;
  G.wpg = wpg;
  G.shared_world = world->n_worlds == 1 ? 1 : 0;
  G.r = r;
  G.policy_params = run->policy_params;
  G.policy_param = run->policy_param;
  G.alpha_f = (float)r.alpha;
  G.gamma_f = (float)r.gamma;
  G.model_lr_f = (float)r.model_lr;
  const auto kernel = r.agent == COBEL_AGENT_DYNAQ ? run_variant<COBEL_AGENT_DYNAQ>(run->policy)
                                                   : run_variant<COBEL_AGENT_Q>(run->policy);
  COBEL_HIP_TRY(cobel_launch(kernel, dim3((unsigned)((r.n + wpg - 1) / wpg)), dim3(64 * wpg), lds, st, G));
  return COBEL_OK;
}

extern "C" int cobel_policy_select_n(int32_t policy, const double* v, const uint8_t* mask_bits,
                                     const double* u_or_null, const uint64_t* k_or_null,
                                     const double* param, int32_t n_param, uint8_t* act, double* probs,
                                     int32_t n, int32_t A, void* stream) {
  const char* const who = "cobel_policy_select_n";
  COBEL_REQUIRE(policy == COBEL_POLICY_SOFTMAX || policy == COBEL_POLICY_EXCLUSIVE ||
                    policy == COBEL_POLICY_RANDOM,
                COBEL_E_ARG, "%s: unknown policy %d (COBEL_POLICY_SOFTMAX, _EXCLUSIVE, _RANDOM)", who,
                policy);
  COBEL_REQUIRE(A >= 1 && A <= kW, COBEL_E_UNSUPPORTED, "%s: %d actions (1 to %d)", who, A, kW);
  COBEL_REQUIRE(n >= 0, COBEL_E_RANGE, "%s: n = %d", who, n);
  if (n == 0) return COBEL_OK;
  const bool random = policy == COBEL_POLICY_RANDOM;
  COBEL_REQUIRE(random ? k_or_null != nullptr : (v && u_or_null && param), COBEL_E_ARG,
                "%s: NULL argument (%s)", who, random ? "RandomDiscrete takes the draws k"
                                                      : "values, draws u and param are required");
  COBEL_REQUIRE(random || n_param == 1 || n_param == n, COBEL_E_ARG,
                "%s: n_param = %d (1 or n = %d)", who, n_param, n);
  COBEL_REQUIRE((((uintptr_t)v | (uintptr_t)u_or_null | (uintptr_t)k_or_null | (uintptr_t)param |
                  (uintptr_t)probs) & 7u) == 0,
                COBEL_E_ARG, "%s: misaligned argument", who);
  hipStream_t st = (hipStream_t)stream;
  if (!random) {
    if (int rc = check_params(policy, param, n_param, st, who)) return rc;
    if (mask_bits)
      if (int rc = check_masks(mask_bits, n, A, "row", st, who)) return rc;
  }
  const long long lanes = (long long)n * kW;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  if (policy == COBEL_POLICY_SOFTMAX)
    hipLaunchKernelGGL(k_policy_select_n<COBEL_POLICY_SOFTMAX>, grid, dim3(256), 0, st, v, mask_bits,
                       u_or_null, k_or_null, param, n_param, act, probs, n, A);
  else if (policy == COBEL_POLICY_EXCLUSIVE)
    hipLaunchKernelGGL(k_policy_select_n<COBEL_POLICY_EXCLUSIVE>, grid, dim3(256), 0, st, v, mask_bits,
                       u_or_null, k_or_null, param, n_param, act, probs, n, A);
  else
    hipLaunchKernelGGL(k_policy_select_n<COBEL_POLICY_RANDOM>, grid, dim3(256), 0, st, v, mask_bits,
                       u_or_null, k_or_null, param, n_param, act, probs, n, A);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}
