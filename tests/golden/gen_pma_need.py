"""Fixture of ``cobel_pma_stationary`` (csrc/pma_need.hip): transition tables T and what the real
reference's ``PMAMemory.compute_need(None)`` (memory/pma.py:403-408) returns for them.

Cases (tests/pma_need_common.py): the worlds small_3x4 (12 states), demo_5x5 (25),
seeded_world(11, 11, 5) (121) and seeded_world(8, 16, 3) (128), each with its initial T and with T
after 10, 60, 400 and 3 000 stores along ``walk_stores(tabs, n, 7)``.  Per case:

  ``T``      float64 [S, S]
  ``need``   float64 [S]: the reference's vector with that T assigned (its first S entries: the
             vector is tiled once per action)
  ``exact``  float64 [S]: the system of pma_need_common solved in ``np.longdouble``, |x| / ||x||_2,
             rounded to float64
  ``gap``    the second-smallest |eig - 1| of T

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_pma_need.py

Reuses the shim of gen_golden.py.  Writes pma_need.npz.
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


def case(world, stores) -> dict:
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    _, sas = pc.tables_of(nc.WORLDS[world]())
    S = sas.shape[0]
    T = nc.case_T(world, stores)
    mem = PMAMemory(sas, EpsilonGreedy(0.1))
    if stores == 0:
        assert np.array_equal(np.asarray(mem.T, dtype=np.float64), T)
    mem.T = T.copy()
    need = np.asarray(mem.compute_need(None), dtype=np.float64)
    assert need.shape == (S * sas.shape[1],) and np.array_equal(need[:S], need[S:2 * S])
    return {'T': T, 'need': need[:S].copy(), 'exact': np.asarray(nc.exact(T), dtype=np.float64),
            'gap': np.float64(nc.eigen_gap(T))}


def main() -> None:
    out = {}
    for world, stores in nc.CASES:
        for k, v in case(world, stores).items():
            out['%s/%s' % (nc.case_name(world, stores), k)] = v
    path = G._out('pma_need.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
