"""Fixture of ``cobel_pma_stationary_wide`` (csrc/pma_need_wide.hip): transition tables T of worlds
beyond the LDS kernel's 128 states and what the real reference's ``PMAMemory.compute_need(None)``
(memory/pma.py:403-408) returns for them.

Cases (tests/pma_need_wide_common.py): seeded_world(3, 43, 10) (129 states), (10, 15, 6) (150),
(13, 17, 6) (221) and (16, 20, 8) (320), each with its initial T and with T after 400 and 3 000
stores along ``walk_stores(tabs, n, 7)``; seeded_world(32, 32, 9) (1 024) initially and after 3 000
stores.  Per case:

  ``T``      float64 [S, S] (not for the 1 024-state world: the tests rebuild it)
  ``need``   float64 [S]: the reference's vector with that T assigned (its first S entries)
  ``exact``  float64 [S]: the system of pma_need_common solved in ``np.longdouble``, |x| / ||x||_2,
             rounded to float64
  ``gap``    the second-smallest |eig - 1| of T

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_pma_need_wide.py

Reuses the shim of gen_golden.py.  Writes pma_need_wide.npz (the 80-bit solves of the two
1 024-state cases take a few minutes).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
sys.path.insert(0, os.path.join(G.ROOT, 'cobel-rl_amd'))
import pma_common as pc  # noqa: E402
import pma_need_common as nc  # noqa: E402
import pma_need_wide_common as wc  # noqa: E402


def case(world, stores) -> dict:
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    _, sas = pc.tables_of(wc.WORLDS[world]())
    S = sas.shape[0]
    T = wc.case_T(world, stores)
    mem = PMAMemory(sas, EpsilonGreedy(0.1))
    if stores == 0:
        assert np.array_equal(np.asarray(mem.T, dtype=np.float64), T)
    mem.T = T.copy()
    need = np.asarray(mem.compute_need(None), dtype=np.float64)
    assert need.shape == (S * sas.shape[1],) and np.array_equal(need[:S], need[S:2 * S])
    out = {'need': need[:S].copy(), 'exact': np.asarray(nc.exact(T), dtype=np.float64),
           'gap': np.float64(nc.eigen_gap(T))}
    if world != wc.BIG:
        out['T'] = T
    return out


def main() -> None:
    out = {}
    for world, stores in wc.CASES:
        for k, v in case(world, stores).items():
            out['%s/%s' % (wc.case_name(world, stores), k)] = v
    path = G._out('pma_need_wide.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
