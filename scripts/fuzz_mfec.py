#!/usr/bin/env python3
"""Randomised parity sweep of the MFEC agent against the NumPy restatement (tests/mfec_common.py):
random graphs (track, grid, hexagonal of random size), capacities, k, epsilon, trial and step counts
and launch shapes (1 to 70 instances, a random one compared), bit for bit: the recorded steps and
estimates, the buffers, the latencies and predict_on_batch.

    python scripts/fuzz_mfec.py [first seed] [count]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 0xC0BE1


def one(seed: int) -> str:
    import mfec_common as mc
    from cobel_amd.agent import MFEC
    from cobel_amd.interface import Topology
    from cobel_amd.interface.simulator.offline import OfflineSimulator
    from cobel_amd.misc import topology_tools as tt
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box
    rng = np.random.default_rng(seed)
    kind = rng.choice(['track', 'grid', 'hex'])
    if kind == 'track':
        nodes, starts = tt.linear_track(int(rng.integers(3, 12)), int(rng.integers(1, 4)), 1.0, 20, 'right')
    elif kind == 'grid':
        nodes, starts = tt.grid(int(rng.integers(3, 9)), (0.0, 1.0))
    else:
        nodes, starts = tt.hexagonal(int(rng.integers(3, 6)), (0.0, 1.0))
    S = len(nodes)
    capacity = int(rng.choice([1, 2, 3, 7, 30, 64, 65, 100, 200]))
    k = int(rng.choice([1, 2, 3, 5, 10, 32]))
    eps = float(rng.choice([0.0001, 0.1, 0.3, 0.6]))
    trials, steps = int(rng.integers(3, 40)), int(rng.integers(2, 60))
    n = int(rng.choice([1, 2, 5, 64, 70]))
    pick, base = int(rng.integers(n)), int(rng.integers(0, 1000))
    D = int(rng.choice([2, 4, 16]))
    obs = {tuple(nodes[key]['pose']): o for key, o in zip(nodes, np.eye(S))}
    env = Topology(nodes, starts, OfflineSimulator(obs, Box(0.0, 1.0, (S,))), n_envs=n, seed=SEED,
                   instance_base=base)
    ag = MFEC(env.observation_space, env.action_space, EpsilonGreedy(eps), capacity=capacity, k=k,
              projection_size=D, rng=np.random.default_rng(seed))
    ag.record_steps, ag.track_instances = trials * steps, True
    try:
        ag.train(env, trials, steps)
    except NotImplementedError as err:      # two nodes whose few random features are allclose
        assert 'allclose' in str(err), err
        return 'seed %d: refused (%s)' % (seed, str(err)[:60])
    w = env._tables()
    tab = {'next': w['next'], 'reward': np.asarray(w['rewards'], dtype=np.float64),
           'terminal': np.asarray(w['terminals']).astype(np.uint8),
           'starts': np.asarray(w['starting_states']).astype(np.uint16)}
    ref, rag = mc.run_restatement(tab, ag.features, [base + pick, trials, steps, capacity, k, 0,
                                                     round(eps * 1e6)], SEED)
    what = 'seed %d: %s S=%d cap=%d k=%d eps=%g n=%d pick=%d' % (seed, kind, S, capacity, k, eps, n, pick)
    rows = ag.recorded_steps(pick)
    assert np.array_equal(rows[:, 0], ref['state']) and np.array_equal(rows[:, 1], ref['action']), what
    assert np.array_equal(rows[:, 4:], ref['q']), what
    assert np.array_equal(ag.monitors.lat_trace.cpu().numpy()[pick], ref['steps']), what
    for b, r in zip(ag.memory(pick).buffers, rag.Q.buffers):
        assert np.array_equal(b.ids, r.ids) and np.array_equal(b.values, r.values), what
        assert np.array_equal(b.times, r.times), what
    got = ag.predict_on_batch(range(S))
    got = got if n == 1 else got[pick].cpu().numpy()
    assert np.array_equal(got, ref['predict']), what
    return what


def main() -> None:
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    for seed in range(first, first + count):
        print('ok', one(seed), flush=True)      # ('ok seed n: refused ...': the world was refused)


if __name__ == '__main__':
    main()
