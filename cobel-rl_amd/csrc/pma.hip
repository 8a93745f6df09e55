// Prioritized Memory Access (Mattar & Daw 2018): PMAMemory.replay / store / update_sr and the trial
// loop of the PMA agent as device calls (cobel_pma_replay, cobel_pma_trial, cobel_pma_store,
// cobel_pma_update_sr).  Every table is float64 and every expression is the reference's, one
// rounding per operation (-ffp-contract=off), sums in NumPy's order.
//
// k_pma_replay / k_pma_trial: one wavefront per instance, one wavefront per workgroup.  Q (the
// working copy), rewards, states, terminals, the action mask, the update mask and the need row stay
// in LDS for the whole launch, beside the utilities of a round and the performed updates (the
// current sequence is a window of them).  A round of a replay:
//   scoring    the lanes stride over the S x A one-step backups (compute_gain_batch); the lanes also
//              take one step each of the extended sequence (compute_gain), lane-uniform code sums
//              the step gains in sequence order
//   selection  utility = gain * need * update_mask, a wave maximum, the tie count by ballots, the
//              uniform, the sequential cumsum(1 / k) / last searched from the right, the ballots
//              again for the position of that tie
//   update     the n-step update_q: targets by lane, applied in sequence order
// k_pma_update_sr: one workgroup of 256 lanes per instance, I - gamma T in LDS, in-place
// Gauss-Jordan without pivoting (up to 128 states; beyond: pma_sr.hip).
// Per-instance parameter sets (cobel_pma_mem_sets_t.param_index): every kernel here is a template over
// SETS.  The form with sets stages the instance's parameters from its set at the top of its body
// (fill_hyper / pma_load_par, cobel_pma.h); the scalar launch takes the form without that code.
// The replay and trial kernels come in two forms, narrow (the default, up to 128 states) and wide
// (COBEL_PMA_WIDE, up to 1 024 states): see pma_narrow / pma_wide below.
//
// Reference behaviour restated (paths relative to the reference's src/cobel):
//   memory/pma.py:148-166 (store), :168-267 (replay), :269-331 (compute_gain), :333-386
//   (compute_gain_batch), :388-411 (compute_need), :413-415 (update_sr), :423-450
//   (action_probs_batch), :452-496 (update_q); agent/pma.py:167-258 (train), :260-317 (test),
//   :319-353 (update_q); policy/greedy.py:40-88
#include <cstring>

#include "cobel_common.h"
#include "cobel_pma.h"
#include "cobel_policy.h"

namespace {

constexpr int kSrThreads = 256;

// The two forms of the replay / trial kernels.  They differ in how a performed update is packed
// into its 32-bit record, in the type that holds a successor state and in the LDS they may ask
// for; every arithmetic expression, summation order and draw is the same code.
//   narrow  state:8 | action:8 | next_state:8 | terminal:8     ns uint8_t    64 KiB
//   wide    state:10 | action:3 | next_state:10 | terminal:9   ns uint16_t  160 KiB
// (selected by COBEL_PMA_WIDE in cobel_pma_mem_t.flags; the narrow form is the default)
struct pma_narrow {
  using ns_t = uint8_t;
  static constexpr int kMaxS = COBEL_PMA_MAX_STATES, kLdsLimit = 64 * 1024;
  static constexpr int kShA = 8, kShN = 16, kShT = 24;
  static constexpr uint32_t kMaskS = 0xffu, kMaskA = 0xffu;
};
struct pma_wide {
  using ns_t = uint16_t;
  static constexpr int kMaxS = COBEL_PMA_WIDE_MAX_STATES, kLdsLimit = 160 * 1024;
  static constexpr int kShA = 10, kShN = 13, kShT = 23;
  static constexpr uint32_t kMaskS = 0x3ffu, kMaskA = 7u;
};

// the LDS of one instance
template <class F>
struct pma_lds {
  double *Q, *R, *U, *need, *sg, *rr;   // [SA] [SA] [SA] [S] [L + 1] [L]
  uint32_t* rec;                        // [L] the performed updates, packed as F says
  typename F::ns_t* ns;                 // [SA]
  uint8_t *tm, *um, *am;                // [SA] [A * S] [S]
};
template <class F>
__host__ __device__ inline size_t pma_lds_carve(unsigned char* base, int S, int A, int L,
                                                pma_lds<F>* out) {
  const size_t SA = (size_t)S * A;
  size_t o = 0;
  pma_lds<F> l;
  l.Q = (double*)(base + o); o += 8 * SA;
  l.R = (double*)(base + o); o += 8 * SA;
  l.U = (double*)(base + o); o += 8 * SA;
  l.need = (double*)(base + o); o += 8 * (size_t)S;
  l.sg = (double*)(base + o); o += 8 * (size_t)(L + 1);
  l.rr = (double*)(base + o); o += 8 * (size_t)(L > 0 ? L : 1);
  l.rec = (uint32_t*)(base + o); o += 8 * (size_t)((L + 2) / 2);
  l.ns = (typename F::ns_t*)(base + o); o += sizeof(typename F::ns_t) * SA;
  l.tm = base + o; o += SA;
  l.um = base + o; o += SA;
  l.am = base + o; o += (size_t)((S + 7) & ~7);
  if (out) *out = l;
  return (o + 15) & ~(size_t)15;
}

struct pma_args {
  cobel_pma_mem_x m;
  int32_t L;
  const int32_t* current_state;
  const double* need;
  const int32_t* force_first;
  cobel_pma_rec_t* records;
};

struct pma_trial_args {
  cobel_pma_mem_x m;
  cobel_pma_run_t r;
  // the world (general.hip: gen_args)
  const cobel_wrec* rec;
  const uint16_t* next_n;
  const float* reward_s;
  const uint8_t* terminal_s;
  const uint16_t* starts;
  const int32_t* start_off;
  const uint32_t* succ_off;
  const uint16_t* succ_state;
  const double* succ_cdf;
  int32_t n_worlds;
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct pma_hyper {
  int S, A, SA;
  uint32_t flags, g, pol_stream;
  uint64_t seed;
  double lrq, gq, mg, eps;   // the memory's, of this instance (pma_load_par)
  double lr, lrT;            // ... what the store takes
  const double *gpow, *gqpow;
};

template <class F>
__device__ __forceinline__ uint32_t mask_of(const pma_lds<F>& l, const pma_hyper& h, bool masked, int s) {
  return masked ? (uint32_t)l.am[s] : 0xffu;
}
template <class F>
__device__ __forceinline__ uint32_t rec_pack(const pma_lds<F>& l, const pma_hyper& h, int idx) {
  const int a = idx / h.S, s = idx - a * h.S;
  const int c = s * h.A + a;
  return (uint32_t)s | ((uint32_t)a << F::kShA) | ((uint32_t)l.ns[c] << F::kShN) |
         ((uint32_t)l.tm[c] << F::kShT);
}
template <class F>
__device__ __forceinline__ int rec_state(uint32_t rc) { return (int)(rc & F::kMaskS); }
template <class F>
__device__ __forceinline__ int rec_action(uint32_t rc) { return (int)((rc >> F::kShA) & F::kMaskA); }
template <class F>
__device__ __forceinline__ int rec_next(uint32_t rc) { return (int)((rc >> F::kShN) & F::kMaskS); }
template <class F>
__device__ __forceinline__ uint32_t rec_terminal(uint32_t rc) { return rc >> F::kShT; }

// One replay of L rounds on the LDS tables (memory/pma.py:199-267).  cm: the memory's draw counter,
// cq: its policy's.  Leaves the performed updates in l.rec / l.rr.
template <class F>
__device__ __forceinline__ void pma_replay_body(const pma_lds<F>& l, const pma_hyper& h, bool masked,
                                                int L, int force_first, uint32_t& cm, uint32_t& cq,
                                                int lane) {
  const int S = h.S, A = h.A, SA = h.SA;
  const bool equal_need = h.flags & COBEL_PMA_EQUAL_NEED, equal_gain = h.flags & COBEL_PMA_EQUAL_GAIN;
  const bool barriers = h.flags & COBEL_PMA_IGNORE_BARRIERS, loops = h.flags & COBEL_PMA_ALLOW_LOOPS;
  const bool original = h.flags & COBEL_PMA_GAIN_ORIGINAL;
  int last_seq = 0;
  for (int upd = 0; upd < L; ++upd) {
    // ---- the sequence to extend ---------------------------------------------------------------
    int ext = -1, base = upd;   // base: first performed update of the candidate sequence
    if (upd > 0) {
      const int es = rec_next<F>(l.rec[upd - 1]);
      ext = es;
      bool loop = false;
      for (int j0 = last_seq; j0 < upd; j0 += 64) {
        const int j = j0 + lane;
        const bool hit = j < upd && rec_state<F>(l.rec[j]) == es;
        loop = loop || (__ballot(hit) != 0ull);
      }
      if (!loop || loops) {
        double q[kMaxA];
        load_row(l.Q, es, A, q);
        const double u = cobel_draw_u01(cq, 0u, h.g, h.pol_stream, h.seed);
        cq += 1u;
        const int ea = cobel_eps_greedy_select_n<double, kMaxA>(q, A, mask_of(l, h, masked, es), u,
                                                                 h.eps, nullptr);
        ext = es + ea * S;
        base = last_seq;
      }
    }
    // ---- gain of the extended sequence (compute_gain), its steps by lane ------------------------
    double ext_gain = 0.0;
    if (ext >= 0 && !equal_gain) {
      l.rec[upd] = rec_pack(l, h, ext);
      l.rr[upd] = l.R[(ext % S) * A + ext / S];
      wsync();
      const int n = upd - base + 1;
      const uint32_t lastrec = l.rec[upd];
      const double fv = max_row(l.Q, rec_next<F>(lastrec), A) * (double)rec_terminal<F>(lastrec);
      for (int j = lane; j < n; j += 64) {
        const uint32_t rc = l.rec[base + j];
        const int st = rec_state<F>(rc), a = rec_action<F>(rc);
        double r = 0.0;
        for (int k = 0; k < n - j; ++k) r += l.rr[base + j + k] * h.gpow[k];
        const double tgt = r + fv * h.gqpow[n - j];
        double q[kMaxA], qn[kMaxA];
        load_row(l.Q, st, A, q);
#pragma unroll
        for (int b = 0; b < kMaxA; ++b) qn[b] = q[b] + h.lrq * ((b == a ? tgt : q[b]) - q[b]);
        double sgn = policy_gain(q, qn, A, mask_of(l, h, masked, st), h.eps, false);
        if (original) sgn = h.mg > sgn ? h.mg : sgn;
        l.sg[j] = sgn;
      }
      wsync();
      for (int j = 0; j < n; ++j) ext_gain += l.sg[j];
      ext_gain = h.mg > ext_gain ? h.mg : ext_gain;
      wsync();
    }
    // ---- scoring: utility = gain * need * update_mask -------------------------------------------
    double mx = -__builtin_huge_val();
    for (int i = lane; i < SA; i += 64) {
      const int a = i / S, s = i - a * S;
      double gain = 1.0;
      if (!equal_gain) {
        if (i == ext) {
          gain = ext_gain;
        } else {
          const int c = s * A + a;
          double q[kMaxA], qn[kMaxA];
          load_row(l.Q, s, A, q);
          const double m = max_row(l.Q, (int)l.ns[c], A);
          const double qa = l.Q[c];
          const double inner = (l.R[c] + (h.gq * m) * (double)l.tm[c]) - qa;
          const double qna = qa + h.lrq * inner;
#pragma unroll
          for (int b = 0; b < kMaxA; ++b) qn[b] = b == a ? qna : q[b];
          gain = policy_gain(q, qn, A, mask_of(l, h, masked, s), h.eps, true);
          gain = gain < h.mg ? h.mg : gain;
        }
      }
      double util = gain * (equal_need ? 1.0 : l.need[s]);
      if (barriers) util = util * (l.um[i] ? 1.0 : 0.0);
      l.U[i] = util;
      mx = util > mx ? util : mx;
    }
    mx = wave_max(mx);
    wsync();
    // ---- selection among the exact ties (Generator.choice: one uniform) ---------------------------
    int k = 0;
    for (int i0 = 0; i0 < SA; i0 += 64) {
      const int i = i0 + lane;
      k += __popcll(__ballot(i < SA && l.U[i] == mx));
    }
    const double u = cobel_draw_u01(cm, COBEL_SUB_DOUBLE, h.g, COBEL_STREAM_PMA_MEMORY, h.seed);
    cm += 1u;
    int chosen = 0;
    if (k > 0) {
      const double p = 1.0 / (double)k;
      double ck = 0.0;
      for (int m = 0; m < k; ++m) ck += p;
      double c = 0.0;
      int passed = 0;
      for (int m = 0; m < k; ++m) {
        c += p;
        if ((m & 63) == lane) passed += (c / ck <= u) ? 1 : 0;
      }
      passed = wave_sum(passed);
      int want = passed + 1 < k ? passed + 1 : k;   // the want-th tie in index order
      for (int i0 = 0; i0 < SA; i0 += 64) {
        const int i = i0 + lane;
        unsigned long long bal = __ballot(i < SA && l.U[i] == mx);
        const int pc = __popcll(bal);
        if (want <= pc) {
          for (int t = 1; t < want; ++t) bal &= bal - 1ull;
          chosen = i0 + (int)__builtin_ctzll(bal);
          break;
        }
        want -= pc;
      }
    }
    if (upd == 0 && force_first >= 0) {
      const uint32_t fa = cobel_draw_bounded(cm, 0u, h.g, COBEL_STREAM_PMA_MEMORY, h.seed, (uint32_t)A);
      cm += 1u;
      chosen = force_first + (int)fa * S;
    }
    // ---- update_q on the chosen sequence, the record ----------------------------------------------
    const int from = chosen == ext ? base : upd;
    wsync();
    l.rec[upd] = rec_pack(l, h, chosen);
    l.rr[upd] = l.R[(chosen % S) * A + chosen / S];
    wsync();
    {
      const int n = upd - from + 1;
      bool abort_all = false;
      if (n > 1)
        for (int j0 = 0; j0 < n; j0 += 64) {
          const int j = j0 + lane;
          abort_all = abort_all || (__ballot(j < n && rec_terminal<F>(l.rec[from + j]) == 0u) != 0ull);
        }
      if (!abort_all) {
        const uint32_t lastrec = l.rec[upd];
        const double fv = max_row(l.Q, rec_next<F>(lastrec), A) * (double)rec_terminal<F>(lastrec);
        for (int j = lane; j < n; j += 64) {
          double r = 0.0;
          for (int kk = 0; kk < n - j; ++kk) r += l.rr[from + j + kk] * h.gqpow[kk];
          l.sg[j] = r + fv * h.gqpow[n - j];
        }
        wsync();
        for (int j = 0; j < n; ++j) {
          const uint32_t rc = l.rec[from + j];
          const int cell = rec_state<F>(rc) * A + rec_action<F>(rc);
          const double qv = l.Q[cell];
          const double td = l.sg[j] - qv;
          const double nv = qv + h.lrq * td;
          wsync();
          if (lane == 0) l.Q[cell] = nv;
          wsync();
        }
      }
    }
    if (ext != chosen) last_seq = upd;
  }
}

// SETS: the form a launch with a param_index takes.  The scalar launch keeps forms without a line
// of the staging from a set — its kernels are the ones they were.
template <bool SETS>
__device__ __forceinline__ void fill_hyper(const cobel_pma_mem_x& m, int i, pma_hyper* h) {
  h->S = m.n_states;
  h->A = m.n_actions;
  h->SA = m.n_states * m.n_actions;
  h->flags = m.flags;
  h->g = m.instance_base + (uint32_t)i;
  h->pol_stream = m.pol_stream;
  h->seed = m.seed;
  // the launch's scalars or the instance's parameter set: here, outside every loop
  pma_par p;
  pma_load_par<SETS>(m, i, &p);
  h->lrq = p.lrq;
  h->gq = p.gq;
  h->mg = p.mg;
  h->eps = p.eps;
  h->lr = p.lr;
  h->lrT = p.lrT;
  h->gpow = p.gpow;
  h->gqpow = p.gqpow;
}

// the instance's tables into LDS (states and terminals clamped to what the layout holds: a table
// edited by hand must not send a row read outside the instance's slice)
template <class F>
__device__ __forceinline__ void load_tables(const cobel_pma_mem_x& m, int i, const pma_lds<F>& l,
                                            const pma_hyper& h, int lane) {
  const size_t off = (size_t)i * h.SA;
  for (int c = lane; c < h.SA; c += 64) {
    l.Q[c] = m.q[off + c];
    l.R[c] = m.rewards[off + c];
    const int ns = m.states[off + c];
    l.ns[c] = (typename F::ns_t)(ns < 0 ? 0 : (ns >= h.S ? h.S - 1 : ns));
    const int tm = m.terminals[off + c];
    l.tm[c] = (uint8_t)(tm < 0 ? 0 : (tm > 255 ? 255 : tm));
    l.um[c] = m.update_mask[off + c];
  }
  for (int s = lane; s < h.S; s += 64) l.am[s] = m.action_mask ? m.action_mask[s] : (uint8_t)0xff;
}
template <class F>
__device__ __forceinline__ void store_records(const pma_lds<F>& l, cobel_pma_rec_t* out, int L,
                                              int lane) {
  for (int j = lane; j < L; j += 64) {
    const uint32_t rc = l.rec[j];
    cobel_pma_rec_t e;
    e.state = (int32_t)rec_state<F>(rc);
    e.action = (int32_t)rec_action<F>(rc);
    e.next_state = (int32_t)rec_next<F>(rc);
    e.terminal = (int32_t)rec_terminal<F>(rc);
    e.reward = l.rr[j];
    out[j] = e;
  }
}

template <class F, bool SETS>
__global__ __launch_bounds__(64) void k_pma_replay(const pma_args P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = (int)threadIdx.x;
  const int i = (int)blockIdx.x;
  const cobel_pma_mem_x& m = P.m;
  pma_hyper h;
  fill_hyper<SETS>(m, i, &h);
  pma_lds<F> l;
  pma_lds_carve(lds_raw, h.S, h.A, P.L, &l);
  load_tables(m, i, l, h, lane);
  int cs = P.current_state ? P.current_state[i] : -1;
  if (cs >= h.S) cs = h.S - 1;
  // (an instance without a state and without a need vector — the host refuses it — reads nothing)
  const double* const nrow = cs >= 0 ? m.SR + ((size_t)i * h.S + cs) * h.S
                                     : (P.need ? P.need + (size_t)i * h.S : nullptr);
  for (int s = lane; s < h.S; s += 64) l.need[s] = nrow ? nrow[s] : 0.0;
  wsync();
  uint32_t cm = m.mem_ctr[i], cq = m.pol_ctr[i];
  int ff = P.force_first ? P.force_first[i] : -1;
  if (ff >= h.S) ff = h.S - 1;
  pma_replay_body(l, h, m.action_mask != nullptr, P.L, ff, cm, cq, lane);
  wsync();
  const size_t off = (size_t)i * h.SA;
  for (int c = lane; c < h.SA; c += 64) m.q[off + c] = l.Q[c];
  store_records(l, P.records + (size_t)i * P.L, P.L, lane);
  if (lane == 0) {
    m.mem_ctr[i] = cm;
    m.pol_ctr[i] = cq;
  }
}

template <class F, bool SETS>
__global__ __launch_bounds__(64) void k_pma_trial(const pma_trial_args G) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = (int)threadIdx.x;
  const int i = (int)blockIdx.x;
  const cobel_pma_mem_x& m = G.m;
  const cobel_pma_run_t& R = G.r;
  pma_hyper h;
  fill_hyper<SETS>(m, i, &h);
  const int S = h.S, A = h.A;
  const uint32_t flags = R.flags;
  const bool learn = flags & COBEL_F_LEARN;
  const bool shared = (flags >> 16) & COBEL_PMA_SHARED_POLICY;
  const bool masked = (flags & COBEL_F_MASK_ACTIONS) && m.action_mask;
  const int L = (learn && !(flags & COBEL_F_NO_REPLAY)) ? R.batch : 0;
  const uint32_t act_stream =
      (flags & COBEL_F_TEST_STREAM) ? COBEL_STREAM_POLICY_TEST : COBEL_STREAM_POLICY;
  if (shared) h.pol_stream = act_stream;
  // the agent's three values: the run's, or those of the instance's set
  double alpha = R.alpha, gpow1 = R.gamma_pow1, act_eps = R.epsilon;
  if constexpr (SETS) {
    int row;
    const pma_set_ptr ps = pma_set_of(m, i, &row);
    if (ps) {
      alpha = pma_uniform(ps->alpha);
      gpow1 = pma_uniform(ps->agent_gamma);
      act_eps = pma_uniform(ps->agent_epsilon);
    }
  }
  pma_lds<F> l;
  pma_lds_carve(lds_raw, S, A, L, &l);
  load_tables(m, i, l, h, lane);

  const int world = (int)(h.g % (uint32_t)G.n_worlds);
  const size_t wbase = (size_t)world * S;
  int32_t* const inst = R.inst + (size_t)i * COBEL_I_WORDS;
  uint32_t ce = (uint32_t)inst[COBEL_I_CTR_ENV];
  uint32_t cp = (uint32_t)inst[COBEL_I_CTR_POLICY];
  uint32_t cm = m.mem_ctr[i], cq = m.pol_ctr[i];
  const int trial = inst[COBEL_I_TRIAL];
  // ---- reset (gridworld.py:142) ---------------------------------------------------------------
  const int start_lo = G.start_off[world];
  const uint32_t start_cnt = (uint32_t)(G.start_off[world + 1] - start_lo);
  int state = (int)G.starts[start_lo + (int)cobel_draw_bounded(ce, 0u, h.g, COBEL_STREAM_ENV,
                                                               h.seed, start_cnt)];
  ce += 1u;
  if (state >= S) state = S - 1;
  // ---- the start-of-trial replay (agent/pma.py:206-213) -----------------------------------------
  if (L > 0) {
    const double* const nrow = m.SR + ((size_t)i * S + state) * S;
    for (int s = lane; s < S; s += 64) l.need[s] = nrow[s];
    wsync();
    uint32_t cx = shared ? cp : cq;
    pma_replay_body(l, h, masked, L, -1, cm, cx, lane);
    cp = shared ? cx : cp;
    cq = shared ? cq : cx;
    wsync();
    if (R.replay_out) store_records(l, R.replay_out + (size_t)i * L, L, lane);
  }
  wsync();
  // ---- the steps (agent/pma.py:214-244), lane-uniform but for the row of T ----------------------
  const size_t off = (size_t)i * h.SA;
  double trew = 0.0;
  int step = 0, last = -1;
  unsigned long long executed = 0;
  for (; step < R.steps_per_trial; ++step) {
    double q[kMaxA];
    load_row(l.Q, state, A, q);
    const double u = cobel_draw_u01(cp, 0u, h.g, act_stream, h.seed);
    cp += 1u;
    const int a = cobel_eps_greedy_select_n<double, kMaxA>(q, A, mask_of(l, h, masked, state), u,
                                                           act_eps, nullptr);
    int ns;
    if (G.succ_off) {
      const double ue = cobel_draw_u01(ce, COBEL_SUB_DOUBLE, h.g, COBEL_STREAM_ENV, h.seed);
      ce += 1u;
      ns = cobel_draw_successor(G.succ_off, G.succ_state, G.succ_cdf, (wbase + (size_t)state) * A + a,
                                ue);
    } else {
      ns = G.rec ? (int)G.rec[wbase + state].next[a] : (int)G.next_n[(wbase + state) * A + a];
    }
    if (ns >= S) ns = S - 1;
    const double r = (double)(G.rec ? G.rec[wbase + ns].reward : G.reward_s[wbase + ns]);
    const uint32_t end = G.rec ? G.rec[wbase + ns].terminal : (uint32_t)G.terminal_s[wbase + ns];
    const int nt = end ? 0 : 1;
    if (learn) {
      const int c = state * A + a;
      // the agent's 1-step update_q (agent/pma.py:329-353)
      const double fv = max_row(l.Q, ns, A) * (double)nt;
      double rs = 0.0;
      rs += r * 1.0;
      double td = rs + fv * gpow1;
      const double qv = l.Q[c];
      td -= qv;
      const double nq = qv + alpha * td;
      // PMAMemory.store (memory/pma.py:158-166)
      const double rv = l.R[c];
      const double nr = rv + h.lr * (r - rv);
      wsync();
      if (lane == 0) {
        l.Q[c] = nq;
        l.R[c] = nr;
        l.ns[c] = (typename F::ns_t)ns;
        l.tm[c] = (uint8_t)nt;
        m.rewards[off + c] = nr;
        m.states[off + c] = ns;
        m.terminals[off + c] = nt;
      }
      double* const Trow = m.T + ((size_t)i * S + state) * S;
      for (int j = lane; j < S; j += 64) {
        const double t = Trow[j];
        Trow[j] = t + h.lrT * ((j == ns ? 1.0 : 0.0) - t);
      }
      wsync();
    }
    trew += r;
    executed += 1ull;
    if (R.occupancy && lane == 0) atomicAdd(R.occupancy + wbase + ns, 1ull);
    state = ns;
    if (end) {
      last = ns;
      break;
    }
  }
  if (step >= R.steps_per_trial) step = R.steps_per_trial - 1;   // logs['steps'] = step
  wsync();
  for (int c = lane; c < h.SA; c += 64) m.q[off + c] = l.Q[c];
  if (lane == 0) {
    if (trial >= 0 && trial < R.trial_cap && R.steps_per_trial > 0) {
      const size_t mo = cobel_mon_offset(R.mon_stripes, R.trial_cap) + (size_t)trial;
      if (R.lat_sum) atomicAdd(R.lat_sum + mo, (unsigned long long)step);
      if (R.lat_cnt) atomicAdd(R.lat_cnt + mo, 1ull);
      if (R.reward_sum) atomicAdd(R.reward_sum + mo, trew);
      if (R.resp_cnt && trew > 0.0) atomicAdd(R.resp_cnt + mo, 1ull);
      if (R.lat_trace) R.lat_trace[(size_t)i * R.trial_cap + trial] = step;
    }
    if (R.last) R.last[i] = last;
    inst[COBEL_I_STATE] = state;
    inst[COBEL_I_STEP] = step;
    inst[COBEL_I_TRIAL] = trial + 1;
    inst[COBEL_I_CTR_ENV] = (int32_t)ce;
    inst[COBEL_I_CTR_POLICY] = (int32_t)cp;
    inst[COBEL_I_FLAGS] = 0;
    *reinterpret_cast<double*>(inst + COBEL_I_REWARD_LO) = trew;
    *reinterpret_cast<unsigned long long*>(inst + COBEL_I_STEPS_LO) += executed;
    if (R.steps_done && executed) atomicAdd(R.steps_done, executed);
    m.mem_ctr[i] = cm;
    if (!shared) m.pol_ctr[i] = cq;
  }
}

// PMAMemory.store, one wavefront per instance: lane 0 the record, the lanes the row of T
template <bool SETS>
__global__ __launch_bounds__(64) void k_pma_store(const cobel_pma_mem_x m,
                                                  const cobel_pma_exp_t* __restrict__ exps) {
  const int lane = (int)threadIdx.x;
  const int i = (int)blockIdx.x;
  const cobel_pma_exp_t e = exps[i];
  const int S = m.n_states, A = m.n_actions;
  pma_par p;
  pma_load_par<SETS>(m, i, &p);
  if (e.state < 0 || e.state >= S || e.action < 0 || e.action >= A || e.next_state < 0 ||
      e.next_state >= S)
    return;
  if (lane == 0) {
    const size_t c = (size_t)i * S * A + (size_t)e.state * A + e.action;
    const double rv = m.rewards[c];
    m.rewards[c] = rv + p.lr * (e.reward - rv);
    m.states[c] = e.next_state;
    m.terminals[c] = e.terminal;
  }
  double* const Trow = m.T + ((size_t)i * S + e.state) * S;
  for (int j = lane; j < S; j += 64) {
    const double t = Trow[j];
    Trow[j] = t + p.lrT * ((j == e.next_state ? 1.0 : 0.0) - t);
  }
}

// SR = inv(I - gamma T): the matrix in LDS, in-place Gauss-Jordan.  Step k: the pivot row is scaled
// by 1 / pivot (the pivot's own place takes 1 / pivot), every other row i loses f = M[i][k] times
// it (its column k takes -f / pivot).  No pivoting: the matrix is strictly diagonally dominant by
// rows, and elimination keeps it so.
template <bool SETS>
__global__ __launch_bounds__(kSrThreads) void k_pma_update_sr(const cobel_pma_mem_x m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int S = m.n_states;
  double* const M = reinterpret_cast<double*>(lds_raw);
  double* const col = M + (size_t)S * S;
  double* const row = col + S;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x;
  const double* const T = m.T + (size_t)i * S * S;
  pma_par p;
  pma_load_par<SETS>(m, i, &p);
  for (int e = t; e < S * S; e += kSrThreads) {
    const int r = e / S, c = e - r * S;
    M[e] = (r == c ? 1.0 : 0.0) - p.gamma * T[e];
  }
  __syncthreads();
  for (int k = 0; k < S; ++k) {
    const double inv = 1.0 / M[k * S + k];
    __syncthreads();
    for (int j = t; j < S; j += kSrThreads) {
      col[j] = M[j * S + k];
      row[j] = (j == k ? 1.0 : M[k * S + j]) * inv;
    }
    __syncthreads();
    for (int e = t; e < S * S; e += kSrThreads) {
      const int r = e / S, c = e - r * S;
      if (r == k) M[e] = row[c];
      else M[e] = (c == k ? 0.0 : M[e]) - col[r] * row[c];
    }
    __syncthreads();
  }
  double* const out = m.SR + (size_t)i * S * S;
  for (int e = t; e < S * S; e += kSrThreads) out[e] = M[e];
}

size_t sr_lds_bytes(int S) { return 8 * ((size_t)S * S + 2 * (size_t)S); }

bool is_wide(const cobel_pma_mem_x& m) { return (m.flags & COBEL_PMA_WIDE) != 0; }
size_t carve_bytes(bool wide, int S, int A, int L) {
  return wide ? pma_lds_carve<pma_wide>(nullptr, S, A, L, nullptr)
              : pma_lds_carve<pma_narrow>(nullptr, S, A, L, nullptr);
}
// update_sr through the blocked kernels (pma_sr.hip): every world past the LDS kernel's, and any
// world under COBEL_DEBUG_PMA_SR=blocked (tests: the two paths agree bit for bit)
bool sr_blocked(int S) {
  if (S > pma_narrow::kMaxS) return true;
  const char* const v = cobel_debug_env("COBEL_DEBUG_PMA_SR");
  return v && !strcmp(v, "blocked");
}

int check_mem(const cobel_pma_mem_x* mem, const char* who, bool replay) {
  COBEL_REQUIRE(mem, COBEL_E_ARG, "%s: NULL mem", who);
  const cobel_pma_mem_x& m = *mem;
  if (is_wide(m))
    COBEL_REQUIRE(m.n_states >= 1 && m.n_states <= pma_wide::kMaxS && m.n_actions >= 1 &&
                      m.n_actions <= kMaxA,
                  COBEL_E_UNSUPPORTED,
                  "%s: %d states, %d actions (PMA serves up to %d states and %d actions, its wide "
                  "form up to %d states)",
                  who, m.n_states, m.n_actions, pma_narrow::kMaxS, kMaxA, pma_wide::kMaxS);
  else
    COBEL_REQUIRE(m.n_states >= 1 && m.n_states <= pma_narrow::kMaxS && m.n_actions >= 1 &&
                      m.n_actions <= kMaxA,
                  COBEL_E_UNSUPPORTED,
                  "%s: %d states, %d actions (PMA serves up to %d states and %d actions)", who,
                  m.n_states, m.n_actions, pma_narrow::kMaxS, kMaxA);
  COBEL_REQUIRE(m.n >= 0, COBEL_E_RANGE, "%s: n = %d", who, m.n);
  COBEL_REQUIRE(m.rewards && m.states && m.terminals && m.T && m.SR, COBEL_E_ARG,
                "%s: rewards, states, terminals, T and SR are required", who);
  COBEL_REQUIRE((((uintptr_t)m.q | (uintptr_t)m.rewards | (uintptr_t)m.T | (uintptr_t)m.SR |
                  (uintptr_t)m.gamma_pow | (uintptr_t)m.gamma_q_pow) & 7u) == 0 &&
                    (((uintptr_t)m.states | (uintptr_t)m.terminals | (uintptr_t)m.mem_ctr |
                      (uintptr_t)m.pol_ctr) & 3u) == 0,
                COBEL_E_ARG, "%s: misaligned table", who);
  if (replay) {
    COBEL_REQUIRE(m.q && m.update_mask && m.mem_ctr && m.pol_ctr && m.gamma_pow && m.gamma_q_pow,
                  COBEL_E_ARG,
                  "%s: q, update_mask, mem_ctr, pol_ctr and the two power tables are required", who);
    // (with an index the scalars are ignored; a set's epsilon is checked where the set is filled)
    COBEL_REQUIRE(m.param_index || (m.epsilon >= 0.0 && m.epsilon <= 1.0), COBEL_E_ARG,
                  "%s: epsilon %g outside [0, 1]", who, m.epsilon);
  }
  return pma_check_sets(m, who);
}

int replay_lds(const cobel_pma_mem_x& m, int L, const char* who, size_t* lds) {
  COBEL_REQUIRE(L >= 0, COBEL_E_RANGE, "%s: replay_length = %d", who, L);
  const bool wide = is_wide(m);
  const int limit = wide ? pma_wide::kLdsLimit : pma_narrow::kLdsLimit;
  *lds = carve_bytes(wide, m.n_states, m.n_actions, L);
  COBEL_REQUIRE(*lds <= (size_t)limit, COBEL_E_UNSUPPORTED,
                "%s: a replay of %d rounds needs %zu B of LDS (%d are served)", who, L, *lds, limit);
  COBEL_REQUIRE(m.pow_len > L, COBEL_E_ARG, "%s: the power tables hold %d entries, %d are needed",
                who, m.pow_len, L + 1);
  return COBEL_OK;
}

}  // namespace

extern "C" int cobel_pma_plan(int32_t n_states, int32_t n_actions, int32_t replay_length,
                              int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_pma_plan: NULL out");
  out[0] = out[1] = out[2] = out[3] = 0;
  COBEL_REQUIRE(n_states >= 1 && n_states <= pma_narrow::kMaxS && n_actions >= 1 &&
                    n_actions <= kMaxA,
                COBEL_E_UNSUPPORTED,
                "cobel_pma_plan: %d states, %d actions (PMA serves up to %d states and %d actions)",
                n_states, n_actions, pma_narrow::kMaxS, kMaxA);
  COBEL_REQUIRE(replay_length >= 0, COBEL_E_RANGE, "cobel_pma_plan: replay_length = %d",
                replay_length);
  const size_t lds = carve_bytes(false, n_states, n_actions, replay_length);
  COBEL_REQUIRE(lds <= (size_t)pma_narrow::kLdsLimit, COBEL_E_UNSUPPORTED,
                "cobel_pma_plan: a replay of %d rounds needs %zu B of LDS (%d are served)",
                replay_length, lds, pma_narrow::kLdsLimit);
  out[0] = (int32_t)lds;
  out[1] = 64;
  out[2] = (int32_t)sr_lds_bytes(n_states);
  out[3] = kSrThreads;
  return COBEL_OK;
}

extern "C" int cobel_pma_plan_wide(int32_t n_states, int32_t n_actions, int32_t replay_length,
                                   int32_t out[4]) {
  COBEL_REQUIRE(out, COBEL_E_ARG, "cobel_pma_plan_wide: NULL out");
  out[0] = out[1] = out[2] = out[3] = 0;
  COBEL_REQUIRE(n_states >= 1 && n_states <= pma_wide::kMaxS && n_actions >= 1 && n_actions <= kMaxA,
                COBEL_E_UNSUPPORTED,
                "cobel_pma_plan_wide: %d states, %d actions (PMA serves up to %d states and %d "
                "actions, its wide form up to %d states)",
                n_states, n_actions, pma_narrow::kMaxS, kMaxA, pma_wide::kMaxS);
  COBEL_REQUIRE(replay_length >= 0, COBEL_E_RANGE, "cobel_pma_plan_wide: replay_length = %d",
                replay_length);
  const size_t lds = carve_bytes(true, n_states, n_actions, replay_length);
  COBEL_REQUIRE(lds <= (size_t)pma_wide::kLdsLimit, COBEL_E_UNSUPPORTED,
                "cobel_pma_plan_wide: %d states, %d actions and a replay of %d rounds need %zu B of "
                "LDS (the wide form serves %d B, the narrow form %d B up to %d states)",
                n_states, n_actions, replay_length, lds, pma_wide::kLdsLimit, pma_narrow::kLdsLimit,
                pma_narrow::kMaxS);
  out[0] = (int32_t)lds;
  out[1] = 64;
  const bool blocked = sr_blocked(n_states);
  out[2] = (int32_t)(blocked ? cobel_pma_sr_blocked_lds() : sr_lds_bytes(n_states));
  out[3] = kSrThreads;
  return COBEL_OK;
}

extern "C" int cobel_pma_replay(const cobel_pma_mem_t* mem_in, int32_t replay_length,
                                const int32_t* current_state, const double* need,
                                const int32_t* force_first, cobel_pma_rec_t* records,
                                void* stream) {
  COBEL_PMA_MEM("cobel_pma_replay");
  if (int rc = check_mem(mem, "cobel_pma_replay", true)) return rc;
  size_t lds = 0;
  if (int rc = replay_lds(*mem, replay_length, "cobel_pma_replay", &lds)) return rc;
  COBEL_REQUIRE(current_state || need, COBEL_E_ARG,
                "cobel_pma_replay: current_state or a need vector is required");
  COBEL_REQUIRE(records || replay_length == 0, COBEL_E_ARG, "cobel_pma_replay: NULL records");
  COBEL_REQUIRE(((uintptr_t)records & 7u) == 0 && ((uintptr_t)need & 7u) == 0 &&
                    (((uintptr_t)current_state | (uintptr_t)force_first) & 3u) == 0,
                COBEL_E_ARG, "cobel_pma_replay: misaligned argument");
  if (mem->n == 0) return COBEL_OK;
  pma_args P;
  P.m = *mem;
  P.L = replay_length;
  P.current_state = current_state;
  P.need = need;
  P.force_first = force_first;
  P.records = records;
  const bool sets = mem->param_index != nullptr;
  COBEL_HIP_TRY(cobel_launch(
      is_wide(*mem) ? (sets ? k_pma_replay<pma_wide, true> : k_pma_replay<pma_wide, false>)
                    : (sets ? k_pma_replay<pma_narrow, true> : k_pma_replay<pma_narrow, false>),
      dim3((unsigned)mem->n), dim3(64), lds, (hipStream_t)stream, P));
  return COBEL_OK;
}

extern "C" int cobel_pma_trial(const cobel_world_t* world, const cobel_pma_mem_t* mem_in,
                               const cobel_pma_run_t* run, void* stream) {
  if (int rc = cobel_world_check(world, "cobel_pma_trial")) return rc;
  COBEL_PMA_MEM("cobel_pma_trial");
  if (int rc = check_mem(mem, "cobel_pma_trial", true)) return rc;
  COBEL_REQUIRE(run && run->inst, COBEL_E_ARG, "cobel_pma_trial: run and run->inst are required");
  COBEL_REQUIRE(world->n_states == mem->n_states && world->n_actions == mem->n_actions,
                COBEL_E_ARG, "cobel_pma_trial: the world has %d states and %d actions, the memory %d and %d",
                world->n_states, world->n_actions, mem->n_states, mem->n_actions);
  COBEL_REQUIRE(run->steps_per_trial >= 0 && run->batch >= 0, COBEL_E_RANGE,
                "cobel_pma_trial: steps_per_trial = %d, batch = %d", run->steps_per_trial, run->batch);
  COBEL_REQUIRE(((uintptr_t)run->inst & 7u) == 0 && ((uintptr_t)run->replay_out & 7u) == 0,
                COBEL_E_ARG, "cobel_pma_trial: misaligned inst / replay_out");
  const bool replays = (run->flags & COBEL_F_LEARN) && !(run->flags & COBEL_F_NO_REPLAY);
  size_t lds = 0;
  if (int rc = replay_lds(*mem, replays ? run->batch : 0, "cobel_pma_trial", &lds)) return rc;
  if (mem->n == 0) return COBEL_OK;
  pma_trial_args G;
  G.m = *mem;
  G.r = *run;
  if (!(run->flags & COBEL_F_MASK_ACTIONS)) G.m.action_mask = nullptr;
  G.rec = world->rec;
  G.next_n = world->next_n;
  G.reward_s = world->reward_s;
  G.terminal_s = world->terminal_s;
  G.starts = world->starts;
  G.start_off = world->start_off;
  G.succ_off = world->succ_off;
  G.succ_state = world->succ_state;
  G.succ_cdf = world->succ_cdf;
  G.n_worlds = world->n_worlds;
  const bool sets = mem->param_index != nullptr;
  COBEL_HIP_TRY(cobel_launch(
      is_wide(*mem) ? (sets ? k_pma_trial<pma_wide, true> : k_pma_trial<pma_wide, false>)
                    : (sets ? k_pma_trial<pma_narrow, true> : k_pma_trial<pma_narrow, false>),
      dim3((unsigned)mem->n), dim3(64), lds, (hipStream_t)stream, G));
  return COBEL_OK;
}

// (the store kernel reads 32-bit states from the experience and writes 32-bit tables: one form)
extern "C" int cobel_pma_store(const cobel_pma_mem_t* mem_in, const cobel_pma_exp_t* experiences,
                               void* stream) {
  COBEL_PMA_MEM("cobel_pma_store");
  if (int rc = check_mem(mem, "cobel_pma_store", false)) return rc;
  COBEL_REQUIRE(experiences && ((uintptr_t)experiences & 7u) == 0, COBEL_E_ARG,
                "cobel_pma_store: experiences must be given, 8-byte aligned");
  if (mem->n == 0) return COBEL_OK;
  hipLaunchKernelGGL(mem->param_index ? k_pma_store<true> : k_pma_store<false>,
                     dim3((unsigned)mem->n), dim3(64), 0, (hipStream_t)stream, *mem, experiences);
  COBEL_HIP_TRY(hipGetLastError());
  return COBEL_OK;
}

extern "C" int cobel_pma_update_sr(const cobel_pma_mem_t* mem_in, void* stream) {
  COBEL_PMA_MEM("cobel_pma_update_sr");
  if (int rc = check_mem(mem, "cobel_pma_update_sr", false)) return rc;
  if (mem->n == 0) return COBEL_OK;
  if (sr_blocked(mem->n_states)) return cobel_pma_sr_blocked(*mem, (hipStream_t)stream);
  COBEL_HIP_TRY(cobel_launch(mem->param_index ? k_pma_update_sr<true> : k_pma_update_sr<false>,
                             dim3((unsigned)mem->n), dim3(kSrThreads),
                             sr_lds_bytes(mem->n_states), (hipStream_t)stream, *mem));
  return COBEL_OK;
}

extern "C" int cobel_pma_param_set_fill(const double memory[7], double alpha, double agent_gamma,
                                        double agent_epsilon, cobel_pma_param_set_t* out) {
  const char* const who = "cobel_pma_param_set_fill";
  COBEL_REQUIRE(out && memory, COBEL_E_ARG, "%s: NULL memory / out", who);
  static_assert(sizeof(cobel_pma_param_set_t) == 80 && sizeof(cobel_pma_param_set_t) % 16 == 0,
                "cobel_pma_param_set_t layout");
  COBEL_REQUIRE(memory[6] >= 0.0 && memory[6] <= 1.0, COBEL_E_ARG,
                "%s: the memory's epsilon %g outside [0, 1]", who, memory[6]);
  COBEL_REQUIRE(agent_epsilon >= 0.0 && agent_epsilon <= 1.0, COBEL_E_ARG,
                "%s: the acting policy's epsilon %g outside [0, 1]", who, agent_epsilon);
  // (update_sr eliminates without pivoting: see k_pma_update_sr)
  COBEL_REQUIRE(memory[3] >= 0.0 && memory[3] < 1.0, COBEL_E_ARG,
                "%s: the memory's gamma %g outside [0, 1)", who, memory[3]);
  out->learning_rate = memory[0];
  out->learning_rate_q = memory[1];
  out->learning_rate_T = memory[2];
  out->gamma = memory[3];
  out->gamma_q = memory[4];
  out->min_gain = memory[5];
  out->epsilon = memory[6];
  out->alpha = alpha;
  out->agent_gamma = agent_gamma;
  out->agent_epsilon = agent_epsilon;
  return COBEL_OK;
}
