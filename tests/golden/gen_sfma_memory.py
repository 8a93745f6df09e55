"""Golden traces of SFMAMemory used on its own, recorded from the real reference.

The reference's memory is filled with ``store()`` and then asked for replays directly
(memory/sfma.py:195-416) — this is how replay is studied.  Every case here is a script of such
calls (tests/sfma_memory_common.py: script_for) on ``sfma_5x5`` / ``sfma_6x7``: about 60 stores
along a seeded walk with one (s, a) stored several times, given TD errors under ``error_mod_local``
/ ``error_mod``, ``decay_strength`` 0.95; replays with the state given, the state ``None`` and
``current_action`` given under each of the seven modes, under ``deterministic`` and ``recency``;
one ``retrieve_random_batch`` with a mask.  Recorded: the calls, every returned experience, C, T, I
and the generator's index after each call, the model tables at the end.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_sfma_memory.py

Reuses the shim, the tape generators and the worlds of gen_golden.py; float32 ``rewards``.  Writes
sfma_memory_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED, STREAM_MEMORY, TapeRNG  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import sfma_memory_common as mc  # noqa: E402

# name: (world, instance, metric, switches set before the first call, switches set before the
#        second half of the stores, stores, repeat, start state)
CASES = {
    'w55_dr_error_local': ('sfma_5x5', 2, 'DR', {'decay_strength': 0.95},
                           {'error_mod_local': True}, 60, (7, 4), 12),
    'w67_sr_error_mod': ('sfma_6x7', 5, 'SR',
                         {'reward_mod_local': True, 'decay_strength': 0.95,
                          'reward_modulation': 0.5},
                         {'error_mod': True, 'state_mod': True}, 64, (11, 3), 21),
}


def metric_of(world, name):
    from cobel.memory.utils import DR, SR, Euclidean
    if name == 'DR':
        return DR(world['width'], world['height'], world['sas'], 0.9, world['invalid_transitions'])
    if name == 'SR':
        return SR(world['sas'], 0.9)
    return Euclidean(world['width'], world['height'])


def run_case(wname, inst, mname, switches, late, n_stores, repeat, start) -> dict:
    from cobel.memory import SFMAMemory
    world = {'sfma_5x5': G.sfma_world_5x5, 'sfma_6x7': G.sfma_world_6x7}[wname]()
    tab = G.compact(world)
    metric = metric_of(world, mname)
    mem = SFMAMemory(metric, world['states'], 4,
                     rng=TapeRNG(SEED, inst, STREAM_MEMORY, double_sub=1))
    mem.rewards = mem.rewards.astype(np.float32)
    stores = mc.walk_stores(tab['next'], tab['reward'], tab['terminal'], tab['starts'], n_stores,
                            seed=inst, repeat=repeat)
    ops = [['set', k, v] for k, v in switches.items()] + mc.script_for(stores, start, G.MODES, late)
    d = mc.run_script(mc.DictMemory(mem, index=lambda m: m.rng.index), ops)
    d['ops'] = mc.dumps(ops)
    d['D'] = np.array(metric.D, dtype=np.float64)
    d['cfg'] = np.array([inst, world['states']], dtype=np.int64)
    return d


def main() -> None:
    out = {}
    for name, case in CASES.items():
        for k, v in run_case(*case).items():
            out['%s/%s' % (name, k)] = v
    path = G._out('sfma_memory_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
