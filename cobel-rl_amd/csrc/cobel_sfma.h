// SFMA kernels: what the LDS-resident form (sfma.hip) and the streaming form (sfma_big.hip) share —
// the launch arguments, the LDS layouts, the DPP reductions and the kernel body itself.
#pragma once
#include "cobel_common.h"
#include "cobel_policy.h"

namespace cobel_sfma {

struct sfma_args {
  const cobel_wrec* rec;
  const uint16_t* starts;
  const int32_t* start_off;
  int32_t S, n_worlds;
  int32_t chunk;  // experiences per lane: ceil(4S / 64)
  cobel_sfma_run_t r;
  cobel_eps_bb eps;
  uint64_t eps_thr[16][3];   // integer CDF thresholds of the unmasked selection (cobel_policy.h)
  float alpha_f, gamma_f, model_lr_f;
  // transition rows that are distributions (cobel_world_set_transitions), else NULL: SFMA.train
  // steps the interface (agent/sfma.py:262-264), whose step() then DRAWS the successor
  // (interface/gridworld.py:119-123) — one double of the env stream per step
  const uint32_t* succ_off;
  const uint16_t* succ_state;
  const double* succ_cdf;
  // streaming form (sfma_big.hip): what the plan keeps in LDS besides the inhibition vector
  uint32_t big_lds;   // kBigNsInLds | kBigRowsInLds
};

// The memory's own calls (sfma_mem.hip: cobel_sfma_store, cobel_sfma_replay) run the same body
// with MEM = 1 (one store per instance) or MEM = 2 (one replay per workgroup, n_replays workgroups
// per instance); `r` then carries the memory's tables and parameters only.
struct sfma_mem_args {
  const cobel_sfma_exp_t* exps;   // MEM 1: [N] the experience to store
  uint32_t* counter;              // [N] next index on the memory stream
  const int32_t* start_state;     // MEM 2: [N] or NULL; < 0: drawn from the clipped strengths
  const int32_t* start_action;    // MEM 2: [N] or NULL; < 0: drawn
  int32_t* lengths;               // MEM 2: [N][n_replays] reactivations of each replay
  double* inhibition;             // MEM 2: [N][S] or NULL, I as replay 0 leaves it
  int32_t n_replays;
  uint32_t mem_flags;             // COBEL_SFM_*
};

constexpr uint32_t kBigNsInLds = 1u;     // NS, the model's successor of every experience
constexpr uint32_t kBigRowsInLds = 2u;   // Dc, Dn, the two similarity rows of a reactivation

struct sfma_lds {
  float4* Q;     // [S]
  double* C;     // [4S] strengths
  double* P;     // [4S] priorities / draw weights of the current reactivation
  double* I;     // [S]  inhibition
  double* Dc;    // [S]  similarity row of the current state
  double* Dn;    // [S]  similarity row of the next state
  float* R;      // [4S] model reward estimate of experience j
  uint16_t* NS;  // [4S] model successor of experience j | nonterminal flag << 15
  double* red;   // [4][max(8, NW)] scratch of the cross-wave reductions (several waves per instance)
  uint64_t* thr; // [48] epsilon-greedy thresholds, entry t * 3 + k
  double* epsc;  // [16] masked selection: base[1..4], bonus[1..4] (cobel_policy.h); then blend,
                 //      interp_fwd, interp_rev, decay_inhibition, i_step, alpha, gamma, beta
                 //      (thr and epsc: the launch's, or those of the instance's parameter set)
};

constexpr int kFastStates = 32;   // 4 S <= 128 experiences, two per lane

__host__ __device__ __forceinline__ size_t sfma_lds_bytes(int S) {
  return (((size_t)S * (16 + 32 + 32 + 8 + 8 + 8 + 16 + 8) + 15) & ~(size_t)15) + 256 + 384 + 128;
}

__device__ __forceinline__ sfma_lds carve(unsigned char* base, int S) {
  sfma_lds L;
  size_t off = 0;
  L.Q = reinterpret_cast<float4*>(base + off);
  off += (size_t)S * 16;
  L.C = reinterpret_cast<double*>(base + off);
  off += (size_t)S * 32;
  L.P = reinterpret_cast<double*>(base + off);
  off += (size_t)S * 32;
  L.I = reinterpret_cast<double*>(base + off);
  off += (size_t)S * 8;
  L.Dc = reinterpret_cast<double*>(base + off);
  off += (size_t)S * 8;
  L.Dn = reinterpret_cast<double*>(base + off);
  off += (size_t)S * 8;
  L.R = reinterpret_cast<float*>(base + off);
  off += (size_t)S * 16;
  L.NS = reinterpret_cast<uint16_t*>(base + off);
  off = (off + (size_t)S * 8 + 15) & ~(size_t)15;
  L.red = reinterpret_cast<double*>(base + off);
  off += 256;
  L.thr = reinterpret_cast<uint64_t*>(base + off);
  off += 384;
  L.epsc = reinterpret_cast<double*>(base + off);
  return L;
}

// The streaming form keeps in LDS what is per state — I always; Dc, Dn and the 2-byte successor
// table as far as the plan finds room — and reads Q, C, the model records and the stamps where the
// caller keeps them.  Its cross-wave scratch holds 16 entries per slot.
__host__ __device__ __forceinline__ size_t sfma_big_lds_bytes(int S, uint32_t what) {
  const size_t per_state = 8 + ((what & kBigRowsInLds) ? 16 : 0) + ((what & kBigNsInLds) ? 8 : 0);
  return (((size_t)S * per_state + 15) & ~(size_t)15) + 512 + 384 + 128;
}

__device__ __forceinline__ sfma_lds carve_big(unsigned char* base, int S, uint32_t what) {
  sfma_lds L;
  size_t off = 0;
  L.Q = nullptr;
  L.C = L.P = nullptr;
  L.R = nullptr;
  L.I = reinterpret_cast<double*>(base + off);
  off += (size_t)S * 8;
  L.Dc = L.Dn = nullptr;
  if (what & kBigRowsInLds) {
    L.Dc = reinterpret_cast<double*>(base + off);
    off += (size_t)S * 8;
    L.Dn = reinterpret_cast<double*>(base + off);
    off += (size_t)S * 8;
  }
  L.NS = reinterpret_cast<uint16_t*>(base + off);
  if (what & kBigNsInLds) off += (size_t)S * 8;
  off = (off + 15) & ~(size_t)15;
  L.red = reinterpret_cast<double*>(base + off);
  off += 512;
  L.thr = reinterpret_cast<uint64_t*>(base + off);
  off += 384;
  L.epsc = reinterpret_cast<double*>(base + off);
  return L;
}

// Cross-lane data movement on the VALU (DPP) instead of ds_bpermute through the LDS crossbar: a
// reactivation is a chain of five dependent wave-wide reductions / scans, so their latency is the
// critical path.  Controls: quad_perm 0x00-0xff, row_shr:n 0x110+n, wave_shr:1 0x138, row_mirror
// 0x140, row_half_mirror 0x141, row_bcast:15 0x142, row_bcast:31 0x143.
// (ZERO_FILL: lanes whose source lane does not exist read 0 — bound_ctrl — instead of keeping
//  `old`: with every row enabled the destination needs no initialisation, two moves less per use)
template <int CTRL, int ROW_MASK = 0xf, bool ZERO_FILL = false>
__device__ __forceinline__ double dpp_f64(double old, double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v), o = __builtin_bit_cast(uint64_t, old);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)o, (int)(uint32_t)b,
                                                            CTRL, ROW_MASK, 0xf, ZERO_FILL);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(o >> 32),
                                                            (int)(uint32_t)(b >> 32), CTRL,
                                                            ROW_MASK, 0xf, ZERO_FILL);
  return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
// max over the wave, returned in every lane (scalar registers)
__device__ __forceinline__ double wave_max_f64(double v) {
  v = fmax(v, dpp_f64<0xB1>(v, v));         // quad_perm [1,0,3,2]
  v = fmax(v, dpp_f64<0x4E>(v, v));         // quad_perm [2,3,0,1]
  v = fmax(v, dpp_f64<0x141>(v, v));        // row_half_mirror
  v = fmax(v, dpp_f64<0x140>(v, v));        // row_mirror: every lane holds its row's max
  v = fmax(v, dpp_f64<0x142, 0xa>(v, v));   // row_bcast:15 into rows 1, 3
  v = fmax(v, dpp_f64<0x143, 0xc>(v, v));   // row_bcast:31 into rows 2, 3
  return readlane_f64(v, 63);
}
// max over the wave of doubles that are >= +0 and not NaN: their order is the order of their bit
// patterns, so the maximum is the largest high word and, among its holders, the largest low word —
// twelve 32-bit DPP maxima instead of six float64 maxima with two DPP moves each.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  // (the compiler keeps DPP move and maximum apart — three instructions per stage; the fused form
  //  needs two wait states after the write of its DPP operand, which inline assembly must supply)
  asm volatile(
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1"
      : "+v"(v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ double wave_max_nonneg_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t hi = (uint32_t)(b >> 32), lo = (uint32_t)b;
  const uint32_t mh = wave_max_u32(hi);
  const uint32_t ml = wave_max_u32(hi == mh ? lo : 0u);
  return __builtin_bit_cast(double, ((uint64_t)mh << 32) | (uint64_t)ml);
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
// inclusive prefix sum over the lanes
__device__ __forceinline__ double wave_scan_f64(double v) {
  v = v + dpp_f64<0x111, 0xf, true>(0.0, v);   // row_shr:1
  v = v + dpp_f64<0x112, 0xf, true>(0.0, v);   // row_shr:2
  v = v + dpp_f64<0x114, 0xf, true>(0.0, v);   // row_shr:4
  v = v + dpp_f64<0x118, 0xf, true>(0.0, v);   // row_shr:8: prefix within each row of 16
  v = v + dpp_f64<0x142, 0xa>(0.0, v);      // rows 1, 3 += last lane of the row before
  v = v + dpp_f64<0x143, 0xc>(0.0, v);      // rows 2, 3 += lane 31
  return v;
}
__device__ __forceinline__ float max4_masked(const float4 q, uint32_t mask) {
  float m = -__builtin_huge_valf();
  if (mask & 1u) m = fmaxf(m, q.x);
  if (mask & 2u) m = fmaxf(m, q.y);
  if (mask & 4u) m = fmaxf(m, q.z);
  if (mask & 8u) m = fmaxf(m, q.w);
  return m;
}

// First experience whose weight equals vmax (np.argmax), wave-uniform.
__device__ __forceinline__ int wave_first_equal(const double* P, int n4, int chunk, int lane,
                                                double vmax) {
  const int j0 = lane * chunk;
  int first = 0x7fffffff;
  for (int k = chunk - 1; k >= 0; --k) {
    const int j = j0 + k;
    if (j < n4 && P[j] == vmax) first = j;
  }
  return wave_min_i32(first);
}

// CH > 0: the common switches (no recency, no C / D normalisation, R normalisation on, softmax
// draw) with exactly CH experiences per lane, which then live in registers from the priority
// rating to the draw.  CH = 0: every switch, any number of experiences per lane, through LDS.
// NW: waves per instance.  1 for the small worlds the reference's demos use; 4 (with CH = 0) for
// worlds of several hundred states, whose 4S experiences would otherwise sit 16-64 deep in each
// lane of a single wave.  Every wave carries the scalar state of the instance redundantly; thread
// 0 does the single-cell writes; the wave-wide reductions are completed across waves through a
// few LDS words and one workgroup barrier each.
// FAST (with CH > 0): the plain training case — learning on, one replay per trial, no start /
// random / dynamic replays, no strength modulation or decay, no per-step host log, occupancy,
// replay trace or per-instance latency trace — with those run-time switches fixed at compile time,
// so that the flags and pointers behind them do not have to stay live across the step loop.
// a / b for many a and one b, given y = 1 / b correctly rounded (one division per reactivation
// instead of one per experience): q0 = RN(a y), r = a - b q0 (exact in an fma), RN(q0 + r y) is the
// correctly rounded quotient (Markstein 1990) — the bits of a / b unless b's significand is all
// ones or the residual leaves the normal range, which the priorities never do.
__device__ __forceinline__ double quotient_by(double a, double b, double y) {
  const double q0 = a * y;
  const double r = __builtin_fma(-q0, b, a);
  return __builtin_fma(r, y, q0);
}

// exp(x) for 0 <= x <= 700 as the device library evaluates it (argument reduction by ln 2 in two
// parts, its degree-11 polynomial, ldexp) without the overflow / underflow selections: the same
// bits for these arguments, six vector instructions fewer per experience.
__device__ __forceinline__ double exp_in_range(double x) {
  const double t = __builtin_rint(x * 0x1.71547652b82fep+0);
  double r = __builtin_fma(t, -0x1.62e42fefa39efp-1, x);
  r = __builtin_fma(t, -0x1.abc9e3b39803fp-56, r);
  double p = __builtin_fma(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
  p = __builtin_fma(r, p, 0x1.71dee623fde64p-19);
  p = __builtin_fma(r, p, 0x1.a01997c89e6b0p-16);
  p = __builtin_fma(r, p, 0x1.a01a014761f6ep-13);
  p = __builtin_fma(r, p, 0x1.6c16c1852b7b0p-10);
  p = __builtin_fma(r, p, 0x1.1111111122322p-7);
  p = __builtin_fma(r, p, 0x1.55555555502a1p-5);
  p = __builtin_fma(r, p, 0x1.5555555555511p-3);
  p = __builtin_fma(r, p, 0x1.000000000000bp-1);
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  return __builtin_ldexp(p, (int)t);
}

// BIG (with CH = 0): the streaming form for worlds whose tables do not fit the LDS.  Q, C, the
// model records and the stamps are read and written in place in the caller's arrays (the waves of a
// workgroup share one vector L1, and every hand-over between threads already has its barrier);
// the priority vector P has no home, so the passes after the first rate their experiences again
// — the same operations in the same order, hence the same float64 values.
// MEM (with CH = 0): SFMAMemory's methods as calls of their own, on the store and the replay of the
// agent's kernel: 1 stores M.exps[i] in instance i and ends; 2 runs one replay of A.r.batch
// reactivations in workgroup (instance, replay) without writing any table of the memory — the
// strengths and the model are read (LDS copy, or in place in the streaming form), inhibition and
// priorities are the workgroup's own — and reports its events, its length and, for replay 0, I.
template <int CH, int NW, bool FAST = false, bool BIG = false, int MEM = 0>
__device__ __forceinline__ void sfma_body(const sfma_args A,
                                          const sfma_mem_args M = sfma_mem_args{}) {
  static_assert(CH == 0 || NW == 1, "the register path is one wave per instance");
  static_assert(!BIG || (CH == 0 && !FAST), "the streaming form is the general path");
  static_assert(MEM == 0 || (CH == 0 && !FAST), "the memory's calls take the general path");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr int NT = 64 * NW;
  constexpr int RS = NW > 8 ? NW : 8;   // entries per slot of the cross-wave scratch
  const bool ns_lds = !BIG || (A.big_lds & kBigNsInLds);
  const bool rows_lds = !BIG || (A.big_lds & kBigRowsInLds);
  const int S = A.S, n4 = 4 * A.S, chunk = A.chunk;
  // (FAST: two experiences per lane means at most kFastStates states — the layout of that many, so
  //  that every LDS address is a compile-time offset instead of ten scalar registers)
  const sfma_lds L = BIG ? carve_big(lds_raw, S, A.big_lds)
                         : (FAST ? carve(lds_raw, kFastStates) : carve(lds_raw, S));
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  // (MEM 2: workgroup b serves replay b % n_replays of instance b / n_replays)
  const int i = MEM == 2 ? (int)blockIdx.x / M.n_replays : (int)blockIdx.x;
  const int rk = MEM == 2 ? (int)blockIdx.x - i * M.n_replays : 0;
  int slot = 0;   // rotating scratch slot: one barrier per cross-wave reduction
  auto bsync = [&]() {
    if (NW == 1) wsync();
    else __syncthreads();
  };
  auto block_max = [&](double v) -> double {
    v = wave_max_f64(v);
    if (NW == 1) return v;
    double* const r = L.red + (slot++ & 3) * RS;
    if (lane == 0) r[wave] = v;
    __syncthreads();
    double m = r[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmax(m, r[w]);
    return m;
  };
  auto block_min_i32 = [&](int v) -> int {
    v = wave_min_i32(v);
    if (NW == 1) return v;
    int* const r = reinterpret_cast<int*>(L.red + (slot++ & 3) * RS);
    if (lane == 0) r[wave] = v;
    __syncthreads();
    int m = r[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = min(m, r[w]);
    return m;
  };
  auto block_sum_i32 = [&](int v) -> int {   // v: one value per wave
    if (NW == 1) return v;
    int* const r = reinterpret_cast<int*>(L.red + (slot++ & 3) * RS);
    if (lane == 0) r[wave] = v;
    __syncthreads();
    int m = r[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m += r[w];
    return m;
  };
  // np.argmax over the weights: the first experience whose weight equals vmax
  // (W(j): the weight of experience j — L.P[j], or its rating over again in the streaming form)
  // (SCAN(F), streaming form: F(j, weight) over this thread's experiences in ascending order)
  auto first_equal = [&](double vmax, auto W, auto SCAN) -> int {
    const int j0 = t * chunk;
    int first = 0x7fffffff;
    if constexpr (BIG) {
      SCAN([&](int j, double w) {
        if (w == vmax) first = min(first, j);
      });
    } else {
      for (int k = chunk - 1; k >= 0; --k) {
        const int j = j0 + k;
        if (j < n4 && W(j) == vmax) first = j;
      }
    }
    return block_min_i32(first);
  };
  // Generator.choice(arange(n4), p = w / sum(w)) for the weights w >= 0 (W(j)), driven by the
  // uniform u: the number of experiences whose cumulative weight is <= u * total.
  // (streaming form: the maximum weight comes out of the summing pass instead of a pass of its
  //  own; `ones`, where given, is set if every weight is zero — np.sum(exp) == 0 -> exp.fill(1) —
  //  and the weights SCAN yields are then all one)
  auto choice = [&](double u, double wmax, auto W, auto SCAN, bool* ones) -> int {
    const int j0 = t * chunk;
    double loc = 0.0;
    if constexpr (BIG) {
      double wm = 0.0;
      SCAN([&](int, double w) {
        loc = loc + w;
        wm = fmax(wm, w);
      });
      wmax = block_max(wm);
      if (ones && !(wmax > 0.0)) {
        *ones = true;
        wmax = 1.0;
        loc = 0.0;
        SCAN([&](int, double w) { loc = loc + w; });
      }
    } else {
      for (int k = 0; k < chunk; ++k)
        if (j0 + k < n4) loc = loc + W(j0 + k);
    }
    const double incl = wave_scan_f64(loc);
    double excl = dpp_f64<0x138, 0xf, true>(0.0, incl);   // wave_shr:1, lane 0 reads 0
    if (NW > 1) {   // add the totals of the waves before this one
      double* const r = L.red + (slot++ & 3) * RS;
      if (lane == 63) r[wave] = incl;
      __syncthreads();
      double off = 0.0;
      for (int w = 0; w < wave; ++w) off = off + r[w];
      excl = off + excl;
    }
    // the cumulative weight at the last experience; threads behind it hold nothing
    double total;
    if (NW == 1) {
      total = readlane_f64(excl + loc, (n4 - 1) / chunk);
    } else {
      double* const r = L.red + (slot++ & 3) * RS;
      if (t == (n4 - 1) / chunk) r[0] = excl + loc;
      __syncthreads();
      total = r[0];
    }
    const double thr = u * total;
    int idx = 0;
    double run = 0.0;
    if constexpr (BIG) {
      int cnt = 0;
      SCAN([&](int, double w) {
        run = run + w;
        cnt += (int)(excl + run <= thr);
      });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
      idx = cnt;
    } else {
      for (int k = 0; k < chunk; ++k) {
        const bool in = j0 + k < n4;
        if (in) run = run + W(j0 + k);
        idx += __popcll(__ballot(in && (excl + run <= thr)));
      }
    }
    idx = block_sum_i32(idx);
    idx = idx < n4 ? idx : n4 - 1;
    // an experience of weight zero has probability zero; rounding at a lane boundary of the scan
    // (or of u * total at u -> 1) is the only way to land on one
    if (!(W(idx) > 0.0)) idx = first_equal(wmax, W, SCAN);
    return idx;
  };
  const uint32_t g = A.r.instance_base + (uint32_t)i;
  const int world = (int)(g % (uint32_t)A.n_worlds);
  const uint4* const W4 = reinterpret_cast<const uint4*>(A.rec + (size_t)world * S);
  const double* const Dm = A.r.metric + (size_t)world * S * S;
  float* const Qg = A.r.q + (size_t)i * n4;
  uint64_t* const Mg = A.r.model + (size_t)i * n4;
  double* const Cg = A.r.strength + (size_t)i * n4;
  uint32_t* const stamp = A.r.stamp + (size_t)i * n4;
  // where a table is read and written: its LDS copy, or (BIG) the caller's array in place
  auto ld_q4 = [&](int s) -> float4 {
    return BIG ? reinterpret_cast<const float4*>(Qg)[s] : L.Q[s];
  };
  auto ld_q = [&](int sa) -> float {
    return BIG ? Qg[sa] : reinterpret_cast<const float*>(L.Q)[sa];
  };
  auto st_q = [&](int sa, float v) {
    if (BIG) Qg[sa] = v;
    else reinterpret_cast<float*>(L.Q)[sa] = v;
  };
  auto ld_c = [&](int j) -> double { return BIG ? Cg[j] : L.C[j]; };
  auto st_c = [&](int j, double v) {
    if (BIG) Cg[j] = v;
    else L.C[j] = v;
  };
  // the model of experience j = a * S + s: successor | nonterminal << 15, reward estimate
  auto ld_ns = [&](int j) -> uint32_t {
    if (ns_lds) return L.NS[j];
    const int a = (int)(j >= S) + (int)(j >= 2 * S) + (int)(j >= 3 * S);
    const uint64_t rec = Mg[(j - a * S) * 4 + a];
    return (uint32_t)(((rec >> 32) & 0x7fffu) | (((rec >> 48) & 1u) << 15));
  };
  auto ld_r = [&](int j) -> float {
    if (!BIG) return L.R[j];
    const int a = (int)(j >= S) + (int)(j >= 2 * S) + (int)(j >= 3 * S);
    return __builtin_bit_cast(float, (uint32_t)Mg[(j - a * S) * 4 + a]);
  };

  // Streaming form: this thread's experiences in ascending order, four at a time (its chunk and 4S
  // are multiples of four, so a group is whole).  The strengths of a group are two 16-byte loads,
  // its stamps one; those of the group after are requested before this one is weighed, and WT4
  // requests what else the four need (similarity, inhibition, successors) before it uses any.
  auto scan4 = [&](bool want_stamps, auto WT4, auto F) {
    const int j0 = t * chunk;
    const int jend = min(j0 + chunk, n4);
    if (j0 >= jend) return;
    int s = j0 % S;
    const double2* cp = reinterpret_cast<const double2*>(Cg + j0);
    const uint4* sp = reinterpret_cast<const uint4*>(stamp + j0);
    double2 ca = cp[0], cb = cp[1];
    uint4 sv = make_uint4(0u, 0u, 0u, 0u);
    if (want_stamps) sv = sp[0];
    for (int j = j0; j < jend; j += 4) {
      const double c[4] = {ca.x, ca.y, cb.x, cb.y};
      const uint32_t st[4] = {sv.x, sv.y, sv.z, sv.w};
      if (j + 4 < jend) {
        cp += 2;
        ca = cp[0];
        cb = cp[1];
        if (want_stamps) sv = *++sp;
      }
      int ss[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ss[k] = s;
        s += 1;
        if (s == S) s = 0;
      }
      double w[4];
      WT4(j, ss, c, st, w);
#pragma unroll
      for (int k = 0; k < 4; ++k) F(j + k, w[k]);
    }
  };

  for (int e = t; e < S; e += NT) {
    if (!BIG && !MEM) L.Q[e] = reinterpret_cast<const float4*>(Qg)[e];
    L.I[e] = 0.0;
  }
  if (t < 48) L.thr[t] = A.eps_thr[t / 3][t % 3];
  if (t < 8) L.epsc[t] = t < 4 ? A.eps.base[t + 1] : A.eps.bonus[t - 3];
  if (t == 8) {
    L.epsc[8] = A.r.blend;
    L.epsc[9] = A.r.interp_fwd;
    L.epsc[10] = A.r.interp_rev;
    L.epsc[11] = A.r.decay_inhibition;
    L.epsc[12] = A.r.i_step;
    L.epsc[13] = A.r.alpha;
    L.epsc[14] = A.r.gamma;
    L.epsc[15] = A.r.beta;
  }
  // Per-instance parameter sets (run.param_index): instance i takes these constants from its set
  // instead of the launch's scalars — here, at the top, and nowhere else.  The plain-training
  // instantiation has no such code: cobel_sfma_run sends a launch with an index to the kernel that
  // serves every value (the conditions of FAST are facts of a set).
  // (a pointer into global memory by its type: were it a generic one, as the copy of the by-value
  //  arguments is, the compiler would merge a scalar's two loads — from the arguments, from the
  //  set — into one load through a selected pointer, and the arguments, 920 B, would then be
  //  copied into scratch in every lane)
  typedef const __attribute__((address_space(1))) cobel_sfma_param_set_t* set_ptr;
  set_ptr PS = nullptr;
  if constexpr (!FAST) {
    if (A.r.param_index) {
      const int k = (int)A.r.param_index[i];
      PS = (set_ptr)(A.r.param_sets + (k < A.r.n_param_sets ? k : A.r.n_param_sets - 1));
      if (t < 48) L.thr[t] = PS->agent.eps_thr[t / 3][t % 3];
      if (t < 8) L.epsc[t] = t < 4 ? PS->agent.eps_base[t + 1] : PS->agent.eps_bonus[t - 3];
      if (t == 8) {
        L.epsc[8] = PS->blend;
        L.epsc[9] = PS->interp_fwd;
        L.epsc[10] = PS->interp_rev;
        L.epsc[11] = PS->decay_inhibition;
        L.epsc[12] = PS->i_step;
        L.epsc[13] = PS->agent.alpha;
        L.epsc[14] = PS->agent.gamma;
        L.epsc[15] = PS->beta;
      }
    }
  }
  if (ns_lds)
    for (int e = t; e < n4; e += NT) {
      if (!BIG) L.C[e] = Cg[e];
      const uint64_t rec = Mg[e];
      const int j = (e & 3) * S + (e >> 2);
      if (!BIG) L.R[j] = __builtin_bit_cast(float, (uint32_t)rec);
      L.NS[j] = (uint16_t)(((rec >> 32) & 0x7fffu) | (((rec >> 48) & 1u) << 15));
    }
  bsync();

  // (MEM: there is no agent; the memory stream continues at M.counter[i], replay rk of a strided
  //  call at its own place (L + 2) * rk behind it — the most one replay can consume)
  int32_t* const inst = MEM ? nullptr : A.r.inst + (size_t)i * COBEL_I_WORDS;
  int32_t* const sinst = A.r.sfma_inst + (size_t)i * COBEL_SI_WORDS;
  int state = MEM ? 0 : inst[COBEL_I_STATE];
  int step = MEM ? 0 : inst[COBEL_I_STEP];
  int trial = MEM ? 0 : inst[COBEL_I_TRIAL];
  uint32_t ce = MEM ? 0u : (uint32_t)inst[COBEL_I_CTR_ENV];
  uint32_t cp = MEM ? 0u : (uint32_t)inst[COBEL_I_CTR_POLICY];
  uint32_t cm = MEM ? M.counter[i] + (uint32_t)rk * (uint32_t)(A.r.batch + 2)
                    : (uint32_t)inst[COBEL_I_CTR_MEMORY];
  uint32_t iflags = MEM ? 0u : (uint32_t)inst[COBEL_I_FLAGS];
  double trew = MEM ? 0.0 : *reinterpret_cast<const double*>(inst + COBEL_I_REWARD_LO);
  unsigned long long nsteps =
      MEM ? 0ull : *reinterpret_cast<const unsigned long long*>(inst + COBEL_I_STEPS_LO);
  uint32_t clock = (uint32_t)sinst[COBEL_SI_CLOCK];
  uint32_t epoch = (uint32_t)sinst[COBEL_SI_EPOCH];
  int mode = sinst[COBEL_SI_MODE];
  uint32_t sflags = (uint32_t)sinst[COBEL_SI_FLAGS];
  double td_acc = *reinterpret_cast<const double*>(sinst + COBEL_SI_TD_LO);
  uint32_t ca = (uint32_t)sinst[COBEL_SI_CTR_AGENT];
  int tpos = A.r.trace_len ? A.r.trace_len[i] : 0;

  const uint32_t flags = A.r.flags, sf = A.r.sfma_flags;
  const bool learn = FAST || (flags & COBEL_F_LEARN);
  const uint32_t pol_stream =
      (flags & COBEL_F_TEST_STREAM) ? COBEL_STREAM_POLICY_TEST : COBEL_STREAM_POLICY;
  const uint8_t* const amask = (flags & COBEL_F_MASK_ACTIONS) ? A.r.action_mask : nullptr;
  const uint64_t seed = A.r.seed;
  const int start_lo = MEM ? 0 : A.start_off[world];
  const uint32_t start_cnt = MEM ? 1u : (uint32_t)(A.start_off[world + 1] - start_lo);
  // Everything in this kernel is wave-uniform, so the compiler wants it all in scalar registers
  // and then spills (1 300 of 3 000 vector instructions were v_readlane / v_writelane).  Constants
  // that only feed vector arithmetic are pinned to vector registers instead.
  double r_thr = A.r.r_threshold;
  float alpha_f = A.alpha_f, gamma_f = A.gamma_f, mlr_f = A.model_lr_f;
  // (what M.store takes: read where it is used without sets, this instance's values with them)
  double dec_str = A.r.decay_strength, c_step = A.r.c_step, rew_mod = A.r.reward_modulation;
  if (PS) {
    r_thr = PS->r_threshold;
    alpha_f = PS->agent.alpha_f;
    gamma_f = PS->agent.gamma_f;
    mlr_f = PS->agent.model_lr_f;
    dec_str = PS->decay_strength;
    c_step = PS->c_step;
    rew_mod = PS->reward_modulation;
  }
  asm volatile("" : "+v"(r_thr), "+v"(alpha_f), "+v"(gamma_f), "+v"(mlr_f));
  // (the constants used once per reactivation or only by some replay modes are read from LDS where
  //  they are used: blend, interp_fwd / _rev, decay_inhibition, i_step, alpha, gamma, beta — L.epsc[8 ..])
  // (the eight constants of the masked action selection sit in LDS: 16 vector registers that decide
  //  between five and six waves per SIMD for the two-experiences-per-lane kernels)
  // cobel_eps_greedy_select_wave (cobel_policy.h) on those scalars: lanes 0..2 take one float64
  // division each, a ballot counts the thresholds of the normalised CDF that u has passed
  auto select_action = [&](const float4 v, uint32_t mask, double u) -> int {
    const float ninf = -__builtin_huge_valf();
    const bool a0 = mask & 1u, a1 = mask & 2u, a2 = mask & 4u, a3 = mask & 8u;
    float m = ninf;
    m = a0 ? fmaxf(m, v.x) : m;
    m = a1 ? fmaxf(m, v.y) : m;
    m = a2 ? fmaxf(m, v.z) : m;
    m = a3 ? fmaxf(m, v.w) : m;
    const bool t0 = a0 && v.x == m, t1 = a1 && v.y == m, t2 = a2 && v.z == m, t3 = a3 && v.w == m;
    const int n = __popc(mask & 15u);
    const int nt = (int)t0 + (int)t1 + (int)t2 + (int)t3;
    const double base = L.epsc[(n <= 1 ? 1 : n) - 1];
    const double bonus = L.epsc[4 + (nt <= 1 ? 1 : nt) - 1];
    const double p0 = a0 ? base + (t0 ? bonus : 0.0) : 0.0;
    const double p1 = a1 ? base + (t1 ? bonus : 0.0) : 0.0;
    const double p2 = a2 ? base + (t2 ? bonus : 0.0) : 0.0;
    const double p3 = a3 ? base + (t3 ? bonus : 0.0) : 0.0;
    const double c0 = p0, c1 = c0 + p1, c2 = c1 + p2, c3 = c2 + p3;
    const double mine = lane == 0 ? c0 : (lane == 1 ? c1 : c2);
    return __popcll(__ballot(lane < 3 && (mine / c3 <= u)));
  };

  // CH > 0: this lane's experiences j = lane * CH + k, their states and whether they exist
  constexpr int CHN = CH > 0 ? CH : 1;
  int jj[CHN], sid[CHN];
  bool inb[CHN];
#pragma unroll
  for (int k = 0; k < CHN; ++k) {
    const int j = t * CHN + k;
    inb[k] = j < n4;
    jj[k] = inb[k] ? j : n4 - 1;
    sid[k] = jj[k] % S;
  }

  cobel_u4 pblk = {0, 0, 0, 0}, mblk = {0, 0, 0, 0};
  uint32_t pb_idx = ~0u, mb_idx = ~0u;
  // scalar double draw number cm of the memory stream (sub 1): one block serves two counters
  auto mem_u01 = [&]() -> double {
    if ((cm >> 1) != mb_idx) {
      mb_idx = cm >> 1;
      mblk = cobel_philox(mb_idx, COBEL_SUB_DOUBLE, g, COBEL_STREAM_MEMORY, seed);
    }
    const double u = (cm & 1u) ? cobel_u01(mblk.z, mblk.w) : cobel_u01(mblk.x, mblk.y);
    cm += 1u;
    return u;
  };
  unsigned long long executed = 0, replayed = 0;
  int budget = A.r.step_budget > 0 ? A.r.step_budget : 0x7fffffff;

  // agent.update_q for a replayed experience (agent/sfma.py:437-455 with M.rewards float32 and
  // M.terminals int64: float64 arithmetic, one rounding into the float32 table)
  auto replay_td = [&](int s, int a, int ns, float R, uint32_t nt) -> double {
    const float4 nrow = ld_q4(ns);
    const float m = max4_masked(nrow, amask ? (uint32_t)amask[ns] & 15u : 15u);
    const float q = ld_q(s * 4 + a);
    const double gnt = L.epsc[14] * (double)nt;
    double td = (double)R + gnt * (double)m;
    td = td - (double)q;
    bsync();
    if (t == 0) st_q(s * 4 + a, (float)((double)q + L.epsc[13] * td));
    bsync();
    td_acc = ((sflags & 1u) ? (double)(float)td_acc : td_acc) + fabs(td);
    sflags &= ~1u;
    return td;
  };
  auto record = [&](int s, int a, int ns, float R, uint32_t nt, int kind, int tr, double td) {
    if (!FAST && A.r.replay_trace && t == 0 && tpos < A.r.trace_cap) {
      cobel_sfma_event_t ev;
      ev.sa = (uint32_t)s | ((uint32_t)a << 16) | (nt << 24) | ((uint32_t)kind << 25);
      ev.next = (uint32_t)ns;
      ev.reward = R;
      ev.trial = tr;
      ev.td = td;
      // (MEM 2: one row of the trace per replay)
      A.r.replay_trace[(size_t)(MEM == 2 ? (int)blockIdx.x : i) * A.r.trace_cap + tpos] = ev;
    }
    tpos += 1;
  };

  // M.store (memory/sfma.py:204-236) of the experience (state, a, r, ns, nt); rd: the reward as the
  // strength modulation takes it, td: the error the error modulation takes (MEM 1 only)
  auto mem_store = [&](int state, int a, int ns, uint32_t nt, float r, double rd, double td) {
    const int sa = state * 4 + a, j = a * S + state;
    const float Rold = ld_r(j);
    const float d = r - Rold;
    const float Rnew = Rold + mlr_f * d;
    if (t == 0) {
      Mg[sa] = cobel_model_pack(Rnew, (uint32_t)ns, nt);   // written through
      if (!BIG) L.R[j] = Rnew;
      if (ns_lds) L.NS[j] = (uint16_t)((uint32_t)ns | (nt << 15));
    }
    if (!FAST && dec_str != 1.0) {
      for (int e = t; e < n4; e += NT) st_c(e, ld_c(e) * dec_str);
      bsync();
    }
    clock += 1u;
    if (t == 0) {
      double c = ld_c(j) + c_step;
      if (!FAST && (sf & COBEL_SF_REWARD_MOD_LOCAL)) c = c + rd * rew_mod;
      st_c(j, c);
      stamp[j] = clock;
    }
    if (!FAST && (sf & COBEL_SF_REWARD_MOD)) {
      bsync();
      const double* const row = Dm + (size_t)state * S;
      for (int e = t; e < n4; e += NT) {
        const int s2 = e % S;
        st_c(e, ld_c(e) + (rd * row[s2]) * rew_mod);
      }
    }
    if constexpr (MEM == 1) {
      // error modulation (:225-233): this experience, then every experience by its similarity to
      // the successor
      if (M.mem_flags & COBEL_SFM_ERROR_MOD_LOCAL) {
        bsync();
        if (t == 0) st_c(j, ld_c(j) + fabs(td));
      }
      if (M.mem_flags & COBEL_SFM_ERROR_MOD) {
        bsync();
        const double* const row = Dm + (size_t)ns * S;
        for (int e = t; e < n4; e += NT) st_c(e, ld_c(e) + fabs(td) * row[e % S]);
      }
    }
    if (!FAST && (sf & COBEL_SF_STATE_MOD)) {
      bsync();
      if (t < 4) st_c(t * S + state, ld_c(t * S + state) + 1.0);
    }
  };

  // SFMAMemory.replay (memory/sfma.py:238-347) [+ the TD updates of SFMA.replay when `update`]
  // (the kernels with experiences in registers are launched without the normalisation switches)
  const bool c_norm = CH == 0 && (sf & COBEL_SF_C_NORMALIZE);
  const bool d_norm = CH == 0 && (sf & COBEL_SF_D_NORMALIZE);
  const int mem_action = (MEM == 2 && M.start_action) ? M.start_action[i] : -1;
  auto sfma_replay = [&](int start_state, bool update, int kind, int tr) {
    int action;
    if (MEM == 2 && mem_action >= 0) {
      action = mem_action;   // current_action given: no integer is drawn (:261-264)
    } else {
      action = (int)cobel_draw_bounded(cm, 0u, g, COBEL_STREAM_MEMORY, seed, 4u);
      cm += 1u;
    }
    int cur = start_state;
    const int j0 = t * chunk;
    if (cur < 0) {
      // no terminal state was reached: start from an experience drawn by strength (:262-270)
      auto w_start = [&](int j) -> double {
        const double c = ld_c(j);
        return c < 0.0 ? 0.0 : c;
      };
      double wmax = 0.0;
      if (!BIG) {
        for (int k = 0; k < chunk; ++k)
          if (j0 + k < n4) {
            const double w = w_start(j0 + k);
            L.P[j0 + k] = w;
            wmax = fmax(wmax, w);
          }
        wmax = block_max(wmax);
      }
      bsync();
      const double u = mem_u01();
      auto start4 = [&](int, const int*, const double* c, const uint32_t*, double* w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = c[k] < 0.0 ? 0.0 : c[k];
      };
      const int pick = choice(
          u, wmax, [&](int j) -> double { return BIG ? w_start(j) : L.P[j]; },
          [&](auto F) { scan4(false, start4, F); }, nullptr);
      action = pick / S;
      cur = pick - action * S;
      bsync();
    }
    int nxt = (int)(ld_ns(action * S + cur) & 0x7fffu);
    for (int e = t; e < S; e += NT) L.I[e] = 0.0;
    double cmax = 1.0;
    if (c_norm) {
      double m = -__builtin_huge_val();
      for (int e = t; e < n4; e += NT) m = fmax(m, ld_c(e));
      cmax = block_max(m);
    }
    bsync();
    const bool need_next = mode == COBEL_SFMA_FORWARD || mode == COBEL_SFMA_BLEND_FORWARD ||
                           mode == COBEL_SFMA_INTERPOLATE || mode == COBEL_SFMA_SWEEPING;
    for (int it = 0; it < A.r.batch; ++it) {
      // similarity rows (:284-287); D_normalize divides the row of the current state only
      const double* const rc = Dm + (size_t)cur * S;
      const double* const rn = Dm + (size_t)nxt * S;
      double dmax = 1.0;
      {
        if (d_norm) {
          double m = -__builtin_huge_val();
          for (int e = t; e < S; e += NT) m = fmax(m, rc[e]);
          dmax = block_max(m);
        }
        if (rows_lds)
          for (int e = t; e < S; e += NT) {
            const double d = rc[e];
            L.Dc[e] = d_norm ? d / dmax : d;
            if (need_next) L.Dn[e] = rn[e];
          }
      }
      bsync();
      // (streaming form beyond the size where two rows fit: the rows are read where they lie)
      auto ld_dc = [&](int s) -> double {
        if (rows_lds) return L.Dc[s];
        const double d = rc[s];
        return d_norm ? d / dmax : d;
      };
      auto ld_dn = [&](int s) -> double { return rows_lds ? L.Dn[s] : rn[s]; };
      int pick;
      if (CH > 0) {
        // similarity of every experience to the one replayed last, by mode (:284-307)
        double d[CHN];
        uint32_t nsv[CHN];
#pragma unroll
        for (int k = 0; k < CHN; ++k) nsv[k] = L.NS[jj[k]] & 0x7fffu;
        switch (mode) {
          case COBEL_SFMA_DEFAULT:
#pragma unroll
            for (int k = 0; k < CHN; ++k) d[k] = L.Dc[sid[k]];
            break;
          case COBEL_SFMA_FORWARD:
#pragma unroll
            for (int k = 0; k < CHN; ++k) d[k] = L.Dn[sid[k]];
            break;
          case COBEL_SFMA_REVERSE:
#pragma unroll
            for (int k = 0; k < CHN; ++k) d[k] = L.Dc[nsv[k]];
            break;
          case COBEL_SFMA_BLEND_FORWARD:
#pragma unroll
            for (int k = 0; k < CHN; ++k) d[k] = L.Dc[sid[k]] + L.epsc[8] * L.Dn[sid[k]];
            break;
          case COBEL_SFMA_BLEND_REVERSE:
#pragma unroll
            for (int k = 0; k < CHN; ++k) d[k] = L.Dc[sid[k]] + L.epsc[8] * L.Dc[nsv[k]];
            break;
          case COBEL_SFMA_INTERPOLATE:
#pragma unroll
            for (int k = 0; k < CHN; ++k)
              d[k] = L.epsc[9] * L.Dn[sid[k]] + L.epsc[10] * L.Dc[nsv[k]];
            break;
          default:
#pragma unroll
            for (int k = 0; k < CHN; ++k) d[k] = L.Dn[nsv[k]];
            break;
        }
        // priority ratings (:308-318)
        double p[CHN];
        double rmax = 0.0;
#pragma unroll
        for (int k = 0; k < CHN; ++k) {
          double R = L.C[jj[k]] * d[k];
          R = R * (1.0 - L.I[sid[k]]);
          if (R < r_thr) R = 0.0;
          p[k] = inb[k] ? R : 0.0;
          rmax = fmax(rmax, p[k]);
        }
        // (FAST: r_threshold >= 0 and strengths, similarities and 1 - I are >= 0 — checked on the
        //  host, resp. true of what the fast launch admits — so the ratings are >= +0)
        rmax = FAST ? wave_max_nonneg_f64(rmax) : block_max(rmax);
        if (!(rmax > 0.0)) break;
        // softmax weights exp(beta R / max R) - 1 (:319-327, :349-372)
        bool some = false;
        const double inv_rmax = 1.0 / rmax;
#pragma unroll
        for (int k = 0; k < CHN; ++k) {
          // (FAST: 0 <= R / max R * beta <= 700 is checked on the host)
          const double x = quotient_by(p[k], rmax, inv_rmax) * L.epsc[15];
          const double w = (FAST ? exp_in_range(x) : exp(x)) + -1.0;
          p[k] = inb[k] ? w : 0.0;
          some = some || p[k] > 0.0;
        }
        if (!__ballot(some)) {  // np.sum(exp) == 0 -> exp.fill(1)
#pragma unroll
          for (int k = 0; k < CHN; ++k) p[k] = inb[k] ? 1.0 : 0.0;
        }
        // the draw: experiences whose cumulative weight is <= u * total
        const double u = mem_u01();
        double loc = p[0];
#pragma unroll
        for (int k = 1; k < CHN; ++k) loc = loc + p[k];
        const double incl = wave_scan_f64(loc);
        const double excl = dpp_f64<0x138, 0xf, true>(0.0, incl);
        const double total = readlane_f64(excl + loc, (n4 - 1) / CHN);
        const double thr = u * total;
        int idx = 0;
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < CHN; ++k) {
          run = run + p[k];
          idx += __popcll(__ballot(inb[k] && (excl + run <= thr)));
        }
        idx = idx < n4 ? idx : n4 - 1;
        bool ok = false;
#pragma unroll
        for (int k = 0; k < CHN; ++k) ok = ok || (inb[k] && jj[k] == idx && p[k] > 0.0);
        if (!__ballot(ok)) {
          // rounding put the draw on an experience of weight zero: take the argmax instead
          double wmax = 0.0;
#pragma unroll
          for (int k = 0; k < CHN; ++k) {
            if (inb[k]) L.P[jj[k]] = p[k];
            wmax = fmax(wmax, p[k]);
          }
          wmax = block_max(wmax);
          bsync();
          idx = wave_first_equal(L.P, n4, CHN, lane, wmax);
        }
        pick = idx;
      } else {
      // priority rating of an experience (:288-316): what it reads, then the arithmetic
      struct sims { double x, y, inh; };
      auto fetch = [&](int j, int s) -> sims {
        sims f;
        f.y = 0.0;
        if (mode == COBEL_SFMA_DEFAULT) f.x = ld_dc(s);
        else if (mode == COBEL_SFMA_FORWARD) f.x = ld_dn(s);
        else if (mode == COBEL_SFMA_REVERSE) f.x = ld_dc(ld_ns(j) & 0x7fffu);
        else if (mode == COBEL_SFMA_BLEND_FORWARD) {
          f.x = ld_dc(s);
          f.y = ld_dn(s);
        } else if (mode == COBEL_SFMA_BLEND_REVERSE) {
          f.x = ld_dc(s);
          f.y = ld_dc(ld_ns(j) & 0x7fffu);
        } else if (mode == COBEL_SFMA_INTERPOLATE) {
          f.x = ld_dn(s);
          f.y = ld_dc(ld_ns(j) & 0x7fffu);
        } else f.x = ld_dn(ld_ns(j) & 0x7fffu);
        f.inh = L.I[s];
        return f;
      };
      auto rate = [&](double c, const sims f, uint32_t st) -> double {
        if (c_norm) c = c / cmax;
        double d;
        if (mode == COBEL_SFMA_BLEND_FORWARD || mode == COBEL_SFMA_BLEND_REVERSE)
          d = f.x + L.epsc[8] * f.y;
        else if (mode == COBEL_SFMA_INTERPOLATE) d = L.epsc[9] * f.x + L.epsc[10] * f.y;
        else d = f.x;
        double R = c * d;
        R = R * (1.0 - f.inh);
        if (sf & COBEL_SF_RECENCY) {
          double t = 0.0;
          if (st > epoch) {
            const uint32_t age = clock - st;
            t = A.r.recency_tab[age < (uint32_t)A.r.recency_len ? age
                                                                  : (uint32_t)A.r.recency_len - 1u];
          }
          R = R * t;
        }
        if (R < r_thr) R = 0.0;
        return R;
      };
      auto rating = [&](int j, int s) -> double {
        const double c = ld_c(j);
        const sims f = fetch(j, s);
        return rate(c, f, (sf & COBEL_SF_RECENCY) ? stamp[j] : 0u);
      };
      auto rating4 = [&](int j, const int* ss, const double* c, const uint32_t* st, double* w) {
        sims f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = fetch(j + k, ss[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = rate(c[k], f[k], st[k]);
      };
      const bool recency = sf & COBEL_SF_RECENCY;
      auto state_of = [&](int j) -> int {
        return j - ((int)(j >= S) + (int)(j >= 2 * S) + (int)(j >= 3 * S)) * S;
      };
      double rmax = 0.0;
      if constexpr (BIG) {
        scan4(recency, rating4, [&](int, double R) { rmax = fmax(rmax, R); });
      } else {
        int s = j0 % S;
        for (int k = 0; k < chunk; ++k) {
          const int j = j0 + k;
          if (j < n4) {
            const double R = rating(j, s);
            L.P[j] = R;
            rmax = fmax(rmax, R);
          }
          s += 1;
          if (s == S) s = 0;
        }
      }
      rmax = block_max(rmax);
      if (!(rmax > 0.0)) break;  // np.sum(R) == 0: nothing left to reactivate (:317-318)
      bsync();
      if (sf & COBEL_SF_DETERMINISTIC) {
        pick = first_equal(
            rmax, [&](int j) -> double { return BIG ? rating(j, state_of(j)) : L.P[j]; },
            [&](auto F) { scan4(recency, rating4, F); });
      } else {
        // softmax(R, offset -1, beta) = exp(beta R) - 1 (:349-372), then the draw
        double wmax = 0.0;
        const double inv_rmax = 1.0 / rmax;
        auto soft = [&](double R) -> double {
          if (sf & COBEL_SF_R_NORMALIZE) R = quotient_by(R, rmax, inv_rmax);
          return exp(R * L.epsc[15]) + -1.0;
        };
        bool ones = false;
        if (!BIG) {
          for (int k = 0; k < chunk; ++k)
            if (j0 + k < n4) {
              const double w = soft(L.P[j0 + k]);
              L.P[j0 + k] = w;
              wmax = fmax(wmax, w);
            }
          wmax = block_max(wmax);
          if (!(wmax > 0.0)) {  // np.sum(exp) == 0 -> exp.fill(1)
            for (int k = 0; k < chunk; ++k)
              if (j0 + k < n4) L.P[j0 + k] = 1.0;
            wmax = 1.0;
          }
        }
        bsync();
        const double u = mem_u01();
        auto soft4 = [&](int j, const int* ss, const double* c, const uint32_t* st, double* w) {
          rating4(j, ss, c, st, w);
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = ones ? 1.0 : soft(w[k]);
        };
        pick = choice(
            u, wmax,
            [&](int j) -> double {
              if (!BIG) return L.P[j];
              return ones ? 1.0 : soft(rating(j, state_of(j)));
            },
            [&](auto F) { scan4(recency, soft4, F); }, &ones);
      }
      }
      action = (int)(pick >= S) + (int)(pick >= 2 * S) + (int)(pick >= 3 * S);   // pick / S
      cur = pick - action * S;
      const uint32_t nrec = ld_ns(pick);
      const float R = ld_r(pick);
      nxt = (int)(nrec & 0x7fffu);
      const uint32_t nt = nrec >> 15;
      bsync();
      // inhibition (:336-337)
      {
        const double dec_inh = L.epsc[11];
        for (int e = t; e < S; e += NT) L.I[e] = L.I[e] * dec_inh;
      }
      bsync();
      if (t == 0) L.I[cur] = fmin(L.I[cur] + L.epsc[12], 1.0);
      // the reactivated experience
      double td = __builtin_nan("");
      if (update) td = replay_td(cur, action, nxt, R, nt);
      record(cur, action, nxt, R, nt, kind, tr, td);
      replayed += 1ull;
      bsync();
    }
  };

  // SFMAMemory.retrieve_random_batch (:374-416) + the TD updates
  auto random_replay = [&](int tr) {
    const int j0 = t * chunk;
    for (int b = 0; b < A.r.batch; ++b) {
      const double u = cobel_draw_u01(cm, COBEL_SUB_DOUBLE + (uint32_t)b, g, COBEL_STREAM_MEMORY,
                                      seed);
      int idx = 0;
      for (int k = 0; k < chunk; ++k)
        idx += __popcll(__ballot(j0 + k < n4 && A.r.random_cdf[j0 + k] <= u));
      idx = block_sum_i32(idx);
      idx = idx < n4 ? idx : n4 - 1;
      const int a = idx / S, s = idx - a * S;   // unravel_index(order='F')
      const uint32_t nrec = ld_ns(idx);
      const int ns = (int)(nrec & 0x7fffu);
      const float R = ld_r(idx);
      const uint32_t nt = nrec >> 15;
      const double td = replay_td(s, a, ns, R, nt);
      record(s, a, ns, R, nt, 0, tr, td);
      replayed += 1ull;
    }
    cm += 1u;   // one vector draw per batch
  };

  // Replays are requested (trial start: one without TD updates; trial end: nb_replays with) and
  // served at ONE place at the top of the loop, so the reactivation code exists once.
  // (Round 4: the replays and the online steps of a trial are inner loops of their own.  As ONE loop
  //  with `continue`s every scalar of either phase was live across every iteration: the online step
  //  reloaded ~140 spilled scalars — v_readlane, a vector instruction on a kernel bound by vector
  //  issue.)
  if constexpr (MEM == 1) {
    // (an experience outside the tables is refused by the callers; here it is left out)
    const cobel_sfma_exp_t x = M.exps[i];
    if ((uint32_t)x.state < (uint32_t)S && (uint32_t)x.action < 4u &&
        (uint32_t)x.next_state < (uint32_t)S)
      mem_store(x.state, x.action, x.next_state, x.nonterminal ? 1u : 0u, (float)x.reward,
                x.reward, x.td);
  }
  if constexpr (MEM == 2) {
    const int s0 = M.start_state ? M.start_state[i] : -1;
    if (s0 < S && mem_action < 4) sfma_replay(s0, false, 0, 0);
    if (t == 0) {
      M.lengths[blockIdx.x] = tpos;
      // a single replay advances the stream by what it drew (a strided call by its whole stride,
      // once every replay has read the counter: cobel_sfma_replay)
      if (!(M.mem_flags & COBEL_SFM_STRIDED)) M.counter[i] = cm;
    }
    if (M.inhibition && rk == 0)
      for (int e = t; e < S; e += NT) M.inhibition[(size_t)i * S + e] = L.I[e];
  }
  int req_count = 0, req_start = -1, req_kind = 0, req_trial = 0;
  while (MEM == 0) {
    while (req_count > 0) {
      req_count -= 1;
      if (!FAST && req_kind == 0 && (sf & COBEL_SF_RANDOM)) random_replay(req_trial);
      else sfma_replay(req_start, req_kind == 0, req_kind, req_trial);
      if (req_count == 0 && req_kind == 0) epoch = clock;  // M.T.fill(0) after a trial's replays
    }
    if (!(iflags & 1u)) {
      if (trial >= A.r.trials_target) break;
      if (budget == 0) break;
      state = (int)A.starts[start_lo + (int)cobel_draw_bounded(ce, 0u, g, COBEL_STREAM_ENV, seed,
                                                               start_cnt)];
      ce += 1u;
      step = 0;
      trew = 0.0;
      iflags |= 1u;
      if (!FAST && learn && (sf & COBEL_SF_START_REPLAY)) {
        req_count = 1;
        req_start = state;
        req_kind = 1;
        req_trial = trial;
        continue;
      }
    }
    // ---- the online steps of the running trial ---------------------------------------------------
    bool out_of_budget = false;
    int ns = state;
    uint32_t end = 0u;
    for (;;) {
    if (budget == 0) {
      out_of_budget = true;
      break;
    }
    budget -= 1;

    // ---- select + env.step ---------------------------------------------------------------------
    const float4 q = ld_q4(state);
    const uint32_t mask_cur = amask ? (uint32_t)amask[state] & 15u : 15u;
    if ((cp >> 1) != pb_idx) {
      pb_idx = cp >> 1;
      pblk = cobel_philox(pb_idx, 0u, g, pol_stream, seed);
    }
    const uint32_t w0 = (cp & 1u) ? pblk.z : pblk.x, w1 = (cp & 1u) ? pblk.w : pblk.y;
    cp += 1u;
    // all actions allowed (no mask, or the reference's default all-true mask): the draw is compared
    // with integer thresholds of the tie pattern's CDF, no floating point (cobel_policy.h) — the
    // float64 selection with its three divisions was 30 % of an online step
    const int a = mask_cur == 15u
                      ? (int)rfl((uint32_t)cobel_eps_greedy_select_thr(q.x, q.y, q.z, q.w,
                                                                        cobel_u53(w0, w1), L.thr, lane))
                      : (int)rfl((uint32_t)select_action(q, mask_cur, cobel_u01(w0, w1)));
    if (!FAST && A.succ_off) {
      const double ue = cobel_draw_u01(ce, COBEL_SUB_DOUBLE, g, COBEL_STREAM_ENV, seed);
      ce += 1u;
      ns = (int)rfl((uint32_t)cobel_draw_successor(
          A.succ_off, A.succ_state, A.succ_cdf, ((size_t)world * S + (size_t)state) * 4 + a, ue));
    } else {
      const uint4 wc = W4[state];
      ns = (int)next_of(rfl(wc.x), rfl(wc.y), a);
    }
    const uint4 wn = W4[ns];
    const float r = __builtin_bit_cast(float, rfl(wn.z));
    end = rfl(wn.w);
    const uint32_t nt = 1u - end;
    float td_online = 0.0f;

    if (learn) {
      const int sa = state * 4 + a;
      mem_store(state, a, ns, nt, r, (double)r, 0.0);
      // agent.update_q online (agent/sfma.py:437-455), float32
      const float4 nrow = ld_q4(ns);
      const float m = max4_masked(nrow, amask ? (uint32_t)amask[ns] & 15u : 15u);
      const float qsa = (a & 2) ? ((a & 1) ? q.w : q.z) : ((a & 1) ? q.y : q.x);
      const float gnt = nt ? gamma_f : 0.0f;
      float td = r + gnt * m;
      td = td - qsa;
      bsync();
      if (t == 0) st_q(sa, qsa + alpha_f * td);
      bsync();
      td_online = td;
      if (sflags & 1u) td_acc = (double)((float)td_acc + fabsf(td));
      else td_acc = td_acc + (double)fabsf(td);
    }

    if (!FAST && A.r.last_exp && t == 0) {
      int32_t* const e = A.r.last_exp + (size_t)i * 6;
      e[0] = state;
      e[1] = a;
      e[2] = ns;
      e[3] = (int32_t)nt;
      e[4] = __builtin_bit_cast(int32_t, r);
      e[5] = __builtin_bit_cast(int32_t, td_online);
    }
    trew += (double)r;
    nsteps += 1ull;
    executed += 1ull;
    if (!FAST && A.r.occupancy && t == 0) atomicAdd(A.r.occupancy + (size_t)world * S + ns, 1ull);
    state = ns;
    if (end || (step + 1 >= A.r.steps_per_trial)) break;
    step += 1;
    }
    if (out_of_budget) break;
    {
      if (t == 0 && trial >= 0 && trial < A.r.trial_cap) {
        const size_t m = cobel_mon_offset(A.r.mon_stripes, A.r.trial_cap) + (size_t)trial;
        if (A.r.lat_sum) atomicAdd(A.r.lat_sum + m, (unsigned long long)step);
        if (A.r.lat_cnt) atomicAdd(A.r.lat_cnt + m, 1ull);
        if (A.r.reward_sum) atomicAdd(A.r.reward_sum + m, trew);
        if (A.r.resp_cnt && trew > 0.0) atomicAdd(A.r.resp_cnt + m, 1ull);
        if (!FAST && A.r.lat_trace) A.r.lat_trace[(size_t)i * A.r.trial_cap + trial] = step;
      }
      const int tr = trial;
      trial += 1;
      iflags &= ~1u;
      if (FAST || (learn && !(flags & COBEL_F_NO_REPLAY))) {
        if (!FAST && (sf & COBEL_SF_DYNAMIC)) {
          // agent/sfma.py:308-316: p(reverse) = 1 / (1 + exp(-(5 td - 2))), in the type the
          // |TD| sum has at this point
          double p0, p1;
          if (sflags & 1u) {
            const float x = (float)td_acc * 5.0f - 2.0f;
            const float p = 1.0f / (1.0f + expf(-x));
            p0 = (double)p;
            p1 = (double)(1.0f - p);
          } else {
            const double x = td_acc * 5.0 - 2.0;
            p0 = 1.0 / (1.0 + exp(-x));
            p1 = 1.0 - p0;
          }
          const double uu = cobel_draw_u01(ca, 0u, g, COBEL_STREAM_AGENT, seed);
          ca += 1u;
          const double c1 = p0 + p1;
          mode = (p0 / c1 <= uu) ? COBEL_SFMA_DEFAULT : COBEL_SFMA_REVERSE;
          td_acc = 0.0;
          sflags |= 1u;
        }
        req_count = FAST ? 1 : A.r.nb_replays;
        req_start = end ? ns : -1;
        req_kind = 0;
        req_trial = tr;
        if (req_count == 0) epoch = clock;  // M.T.fill(0)
      }
    }
  }

  bsync();
  if (!BIG) {
    if (!MEM)
      for (int e = t; e < S; e += NT) reinterpret_cast<float4*>(Qg)[e] = L.Q[e];
    if (MEM != 2)
      for (int e = t; e < n4; e += NT) Cg[e] = L.C[e];
  }
  if (MEM == 1 && t == 0) sinst[COBEL_SI_CLOCK] = (int32_t)clock;
  if (!MEM && t == 0) {
    inst[COBEL_I_STATE] = state;
    inst[COBEL_I_STEP] = step;
    inst[COBEL_I_TRIAL] = trial;
    inst[COBEL_I_CTR_ENV] = (int32_t)ce;
    inst[COBEL_I_CTR_POLICY] = (int32_t)cp;
    inst[COBEL_I_CTR_MEMORY] = (int32_t)cm;
    inst[COBEL_I_FLAGS] = (int32_t)iflags;
    *reinterpret_cast<double*>(inst + COBEL_I_REWARD_LO) = trew;
    *reinterpret_cast<unsigned long long*>(inst + COBEL_I_STEPS_LO) = nsteps;
    sinst[COBEL_SI_CLOCK] = (int32_t)clock;
    sinst[COBEL_SI_EPOCH] = (int32_t)epoch;
    sinst[COBEL_SI_MODE] = mode;
    sinst[COBEL_SI_FLAGS] = (int32_t)sflags;
    *reinterpret_cast<double*>(sinst + COBEL_SI_TD_LO) = td_acc;
    sinst[COBEL_SI_CTR_AGENT] = (int32_t)ca;
    if (A.r.trace_len) A.r.trace_len[i] = tpos;
    if (A.r.steps_done && executed) atomicAdd(A.r.steps_done, executed);
    if (A.r.replays_done && replayed) atomicAdd(A.r.replays_done, replayed);
  }
}

// What cobel_sfma_run and the memory's calls refuse of per-instance parameter sets before a launch:
// an index without sets, a number of sets a 16-bit index cannot address, misaligned pointers.
// Without an index the other two fields are not looked at.
inline int sfma_check_sets(const cobel_sfma_param_set_t* sets, const uint16_t* index,
                           int32_t n_sets, const char* who) {
  if (!index) return COBEL_OK;
  COBEL_REQUIRE(sets, COBEL_E_ARG, "%s: param_index given without parameter sets", who);
  COBEL_REQUIRE(n_sets >= 1 && n_sets <= 65535, COBEL_E_RANGE,
                "%s: %d parameter sets (1 ... 65535)", who, n_sets);
  COBEL_REQUIRE(((uintptr_t)sets & 15u) == 0 && ((uintptr_t)index & 1u) == 0, COBEL_E_ARG,
                "%s: param_sets must be 16-byte, param_index 2-byte aligned", who);
  return COBEL_OK;
}

// sfma_big.hip: the streaming form, `threads` (256 or 1 024) per instance
int launch_sfma_big(const sfma_args& A, int threads, size_t lds, hipStream_t st);

}  // namespace cobel_sfma
