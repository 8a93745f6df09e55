// The replay batch of a DQN act step drawn from the ring (memory/dqn.py:137: uniform over the stored
// entries, with replacement), one lane per (instance, sample): sub-stream j of ONE counter of the
// memory stream — the value the act kernel has just counted past.  Shared by cobel_dqn_act
// (dqn_act.hip) and cobel_dqn_act_c2d (dqn_act_c2d.hip), whose structs name the fields alike.
#ifndef COBEL_DQN_BATCH_H
#define COBEL_DQN_BATCH_H

#include "cobel_common.h"

// R: cobel_dqn_act_t or cobel_dqn_c2d_act_t (ring, stepped, memory_ctr, batch, slots); tid: the
// lane's number in the launch; n, instance_base, seed: of the run (the arena's, on the arena)
template <typename RUN>
__device__ __forceinline__ void cobel_dqn_ring_batch(const RUN& R, long long tid, int n,
                                                     uint32_t instance_base, uint64_t seed) {
  const int i = (int)(tid / R.batch), j = (int)(tid - (long long)i * R.batch);
  if (i >= n || !R.stepped[i]) return;
  const uint32_t g = instance_base + (uint32_t)i;
  const uint32_t mc = R.memory_ctr[i] - 1u;
  const int size = R.ring_size[i], slots = R.slots;
  const long long head = R.ring_head[i];
  const uint32_t idx = cobel_draw_bounded(mc, (uint32_t)j, g, COBEL_STREAM_MEMORY, seed,
                                          (uint32_t)size);
  R.batch_slots[(size_t)i * R.batch + j] = (int32_t)((head + (long long)idx) % slots);
}

#endif  // COBEL_DQN_BATCH_H
