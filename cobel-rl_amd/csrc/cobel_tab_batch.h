// The planning / replay batch of the wavefront tabular kernels k_tab_wpi and k_tab_wqn: B
// sequential TD updates, lane j < n holding update j, run as speculative rounds.  (k_tab_pwg's LDS
// waves run the same scheme written out in tabular_pwg.hip: see there.)
//
// The reference applies the updates one after another (agent/dyna_q.py:327-330, agent/q.py:
// 344-354).  Lane j may commit once every earlier lane that writes a cell j reads — its own cell
// or a cell of the row it maximises over — has written.  The rounds are speculative: every
// remaining lane computes its update from the table as it stands; its result holds unless an
// earlier lane of this round that writes a cell it reads has CHANGED that cell — an update that
// leaves its cell as it was (all-zero regions of Q, converged entries) blocks nobody.
//
// Who is held back is found IN the table (tags): a lane that changes its cell raises it to the
// tag ~lane with ds_max_u32.  Tags are the bit patterns 0xffffffc0 .. 0xffffffff, above every
// float (the -inf of pad cells included) that is not a NaN of exactly that payload, so the cell
// then holds the tag of the EARLIEST lane that writes it.  Every lane reads its row and its cell
// again and is held back iff one of them holds a tag above its own: an earlier writer of a cell it
// reads.  The earliest writer of a cell then stores the new value (committed) or puts the old one
// back (held back): only changed cells are written, once per round.  The lanes before the first
// held-back one are committed, the rest go again.  Same order of effects as the reference's loop,
// exact for any state count, no byte of LDS beside the table.
//
// The first lane of a round (`lo`) is committed regardless.  Only a table that held a tag pattern
// to begin with — a NaN no arithmetic produces — could hold it back: garbage in, garbage out, but
// every round ends one lane further and every batch ends.
//
// The first round is written out in front of the loop over the rounds: most batches end with it
// (91 % on trained agents, scripts/experiments/exp_pwg_hist.py), and as the loop's first trip it
// carried the loop's masks and round state (k_tab_pwg: 12.27 -> 12.06 ms per C3 launch; k_tab_wpi
// on trained 16 x 16 / 24 x 24 mazes +1.3 / +0.7 %, scripts/experiments/exp_occ_trained.py).
//
// Every access to the table in here is a 32-bit integer access; the arithmetic works on the bits
// cast to float.  Every hand-off between lanes is a wsync().
#pragma once
#include "cobel_common.h"

// The maximum of a row of W values, as each kernel has always computed it (max4's v_max3 pair and
// fmaxf differ on NaNs and on the sign of a zero: the two are not interchangeable).
template <int W>
__device__ __forceinline__ float cobel_row_max(const uint4* const row) {
  auto f4 = [](const uint4 v) -> float4 {
    return make_float4(__builtin_bit_cast(float, v.x), __builtin_bit_cast(float, v.y),
                       __builtin_bit_cast(float, v.z), __builtin_bit_cast(float, v.w));
  };
  if (W == 4) return max4(f4(row[0]));
  // (rows of 8 / 16 / 32, pad cells -inf)
  float4 v = f4(row[0]);
  float m = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
  for (int j = 1; j < W / 4; ++j) {
    v = f4(row[j]);
    m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
  }
  return m;
}

// Q: the table, rows of W words.  cell: the cell this lane updates; ns: the row it maximises over.
// on: the lane takes part (lane < n; a constant true where the caller already runs under it).
// n: the updates of the batch (lanes 0 .. n - 1).  td(q, row max): the updated value of the cell.
template <int W, typename TD>
__device__ __forceinline__ void cobel_tab_batch(uint32_t* const Q, const uint32_t cell,
                                                const uint32_t ns, const bool on, const int n,
                                                const int lane, TD&& td) {
  static_assert(W == 4 || W == 8 || W == 16 || W == 32, "rows of 4, 8, 16 or 32 words");
  const uint4* const row = reinterpret_cast<const uint4*>(Q) + ns * (uint32_t)(W / 4);
  const uint32_t tag_mine = ~(uint32_t)lane;
  // this lane's update from the table as it stands: q = the cell, returns the new value
  auto update = [&](float& q) -> float {
    const float m = cobel_row_max<W>(row);
    q = __builtin_bit_cast(float, Q[cell]);
    return td(q, m);
  };
  // tags raised, inputs read again, the round's committed lanes [.., stop) settled; returns stop
  auto settle = [&](bool act, bool ch, float q, float qn, int lo) -> int {
    if (ch) atomicMax(&Q[cell], tag_mine);
    wsync();
    uint32_t t = 0u, c2 = 0u;
    if (act) {
      c2 = Q[cell];
      t = c2;
#pragma unroll
      for (int j = 0; j < W / 4; ++j) {
        const uint4 v = row[j];
        t = max(max(max(v.x, v.y), v.z), max(v.w, t));
      }
    }
    const unsigned long long blocked = __builtin_amdgcn_ballot_w64(act && t > tag_mine);
    const int stop = max(blocked ? __ffsll((long long)blocked) - 1 : n, lo + 1);
    if (ch && c2 == tag_mine) Q[cell] = fbits(lane < stop ? qn : q);
    wsync();
    return stop;
  };
  int first;
  {
    float q = 0.0f, qn = 0.0f;
    if (on) qn = update(q);
    const bool ch = on && fbits(qn) != fbits(q);
    if (!__builtin_amdgcn_ballot_w64(ch)) return;
    first = settle(on, ch, q, qn, 0);
  }
  while (first < n) {
    const bool act = on && lane >= first;
    float q = 0.0f, qn = 0.0f;
    if (act) qn = update(q);
    const bool ch = act && fbits(qn) != fbits(q);
    if (!__ballot(ch)) return;
    first = settle(act, ch, q, qn, first);
  }
}
