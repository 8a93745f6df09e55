"""Golden values of PMAMemory's observables, recorded from the real reference in float64:
``compute_gain_batch``, ``compute_gain``, ``action_probs_batch`` and ``update_q``
(memory/pma.py:269-386, :423-496) on the cases of tests/pma_gain_common.py — five worlds (3 x 4,
5 x 5, an eight-action and a one-action table, 12 x 11), three memories each filled by a different
seeded walk of ``store()`` calls, with and without an action mask, on Q tables that are all zero,
random, tied, and that do and do not change the greedy action under a one-step backup; hand-built
n-step updates of 1 .. 256 steps in both ``min_gain_mode``s with ``gamma`` 0.9 and ``gamma_q`` 0.99.
Besides, ``action_probs_batch`` on tables of 1 .. 257 rows and 1, 4 and 8 actions.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_pma_gain.py

Reuses the shim of gen_golden.py.  Writes pma_gain.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
sys.path.insert(0, os.path.join(G.ROOT, 'cobel-rl_amd'))
import pma_gain_common as gc  # noqa: E402


def reference_memories(case: dict, mode: str) -> list:
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    mems = []
    for i in range(gc.N):
        mem = PMAMemory(case['sas'], EpsilonGreedy(gc.EPS, rng=np.random.default_rng(0)),
                        gamma=gc.GAMMA, gamma_q=gc.GAMMA_Q, rng=np.random.default_rng(0))
        mem.min_gain_mode = mode
        for row in case['stores'][i]:
            mem.store(gc.exp(row))
        mems.append(mem)
    return mems


def main() -> None:
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    out = {}
    for name in gc.WORLDS:
        case = gc.build(name)
        got = gc.observables(case, lambda mode: reference_memories(case, mode), real=True)
        for k, v in got.items():
            out['%s/%s' % (name, k)] = v
    probe = PMAMemory(gc.build('small_3x4')['sas'], EpsilonGreedy(gc.EPS, rng=np.random.default_rng(0)))
    for rows in gc.PROB_ROWS:
        for A in gc.PROB_ACTIONS:
            for masked in (False, True):
                q, mask = gc.prob_case(rows, A, masked)
                out['probs/%dx%d/%s' % (rows, A, gc.MASKS[masked])] = probe.action_probs_batch(q, mask)
    path = G._out('pma_gain.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
