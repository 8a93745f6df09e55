#!/usr/bin/env python3
"""Randomised parity sweep of the MFEC agent against the NumPy restatement (tests/mfec_common.py):
random graphs (track, grid, hexagonal of random size), capacities, k, epsilon, trial and step counts
and launch shapes (1 to 70 instances, a random one compared), bit for bit: the recorded steps and
estimates, the buffers, the latencies and predict_on_batch.

    python scripts/fuzz_mfec.py [first seed] [count]

Seeds from 10^6 on draw from the top of the documented ranges instead: random graphs of 100 to
1 024 nodes with 5 to 8 neighbours, capacities of 64 to 2 048, k up to 32, and lattice, one-hot or
random features given to the agent as its feature table (exact ties; tests/mfec_limits_common.py).

A world in which two nodes' few random features are allclose is refused by the agent; such a seed is
left out and listed in ``REFUSED``.  tests/test_gpu_fuzz_agents.py runs a fixed slice of each range.
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
REFUSED: list = []      # seeds whose world the agent refused (allclose features)


WIDE = 1_000_000        # first seed of the second range


def draw_wide_case(seed: int) -> dict:
    rng = np.random.default_rng(seed)
    size = (int(rng.integers(100, 1025)), int(rng.integers(5, 9)))
    capacity = int(rng.choice([64, 65, 128, 300, 2048]))
    k = int(rng.choice([1, 2, 3, 5, 10, 32]))
    eps = float(rng.choice([0.1, 0.3, 0.6]))
    trials, steps = int(rng.integers(20, 90)), int(rng.integers(20, 80))
    n = int(rng.choice([1, 2, 65]))
    pick, base = int(rng.integers(n)), int(rng.integers(0, 1000))
    features = str(rng.choice(['lattice', 'onehot', 'random']))
    goals = int(rng.integers(size[0] // 60 + 1, size[0] // 25 + 2))
    return dict(seed=seed, kind='graph', size=size, capacity=capacity, k=k, eps=eps, trials=trials,
                steps=steps, n=n, pick=pick, base=base, D={'lattice': 2, 'onehot': size[0]}.get(features, 16),
                features=features, goals=goals)


def draw_case(seed: int) -> dict:
    if seed >= WIDE:
        return draw_wide_case(seed)
    rng = np.random.default_rng(seed)
    kind = str(rng.choice(['track', 'grid', 'hex']))
    if kind == 'track':
        size = (int(rng.integers(3, 12)), int(rng.integers(1, 4)))
    elif kind == 'grid':
        size = (int(rng.integers(3, 9)),)
    else:
        size = (int(rng.integers(3, 6)),)
    capacity = int(rng.choice([1, 2, 3, 7, 30, 64, 65, 100, 200]))
    k = int(rng.choice([1, 2, 3, 5, 10, 32]))
    eps = float(rng.choice([0.0001, 0.1, 0.3, 0.6]))
    trials, steps = int(rng.integers(3, 40)), int(rng.integers(2, 60))
    n = int(rng.choice([1, 2, 5, 64, 70]))
    pick, base = int(rng.integers(n)), int(rng.integers(0, 1000))
    D = int(rng.choice([2, 4, 16]))
    return dict(seed=seed, kind=kind, size=size, capacity=capacity, k=k, eps=eps, trials=trials,
                steps=steps, n=n, pick=pick, base=base, D=D)


def world_of(c: dict):
    """(nodes, starting nodes) of a case."""
    from cobel_amd.misc import topology_tools as tt
    if c['kind'] == 'graph':
        import mfec_limits_common as ml
        return ml.random_graph(c['size'][0], c['size'][1], c['seed'], goals=c['goals'])
    if c['kind'] == 'track':
        return tt.linear_track(c['size'][0], c['size'][1], 1.0, 20, 'right')
    if c['kind'] == 'grid':
        return tt.grid(c['size'][0], (0.0, 1.0))
    return tt.hexagonal(c['size'][0], (0.0, 1.0))


def tables_of(nodes, starts) -> dict:
    """The compact tables of a Topology over these nodes (interface/topology.py, ``_tables``), in the
    restatement's names."""
    ids = list(nodes.keys())
    index = {key: i for i, key in enumerate(ids)}
    return {'next': np.array([[index[m] for m in nodes[key]['neighbors']] for key in ids], dtype=np.uint16),
            'reward': np.array([nodes[key]['reward'] for key in ids], dtype=np.float64),
            'terminal': np.array([bool(nodes[key]['terminal']) for key in ids]).astype(np.uint8),
            'starts': np.array([index[key] for key in starts]).astype(np.uint16)}


def features_of(c: dict, S: int) -> np.ndarray:
    """The agent's feature table: one-hot observations times the projection its generator draws
    first (agent/mfec.py: ``rng.random((S, projection_size))``) — the projection's rows.  The second
    range names its table (``feature_table`` is overridden with it)."""
    if c['kind'] == 'graph':
        import mfec_limits_common as ml
        return ml.features(c['features'], S, c['seed'])
    return np.dot(np.eye(S), np.random.default_rng(c['seed']).random((S, c['D'])))


def run_reference(c: dict):
    """-> (record, restated agent, tables), or (None, None, tables) for a world that is refused."""
    import mfec_common as mc
    nodes, starts = world_of(c)
    tab = tables_of(nodes, starts)
    F = features_of(c, len(nodes))
    more = {}
    if c['kind'] == 'graph':    # (forms shown equal to the plain ones in tests/test_host_mfec.py)
        import mfec_limits_common as ml
        tables, more = ml.tables(c['features'], len(nodes), c['seed'])[1], {'query': ml.tree_query}
    else:
        tables = mc.pair_tables(F)
    if (tables[1] & ~np.eye(len(nodes), dtype=bool)).any():
        return None, None, tab
    ref, rag = mc.run_restatement(tab, F, [c['base'] + c['pick'], c['trials'], c['steps'],
                                           c['capacity'], c['k'], 0, round(c['eps'] * 1e6)], SEED,
                                  tables=tables, **more)
    return ref, rag, tab


def describe(c: dict) -> str:
    return ('seed %(seed)d: %(kind)s %(size)s cap=%(capacity)d k=%(k)d eps=%(eps)g trials=%(trials)d '
            'steps=%(steps)d n=%(n)d pick=%(pick)d base=%(base)d D=%(D)d' % c
            + (' %(features)s goals=%(goals)d' % c if c['kind'] == 'graph' else ''))


def run_case(c: dict) -> list:
    """The mismatches of a case (none: it agrees, or its world was refused: see ``REFUSED``)."""
    from cobel_amd.agent import MFEC
    from cobel_amd.interface import Topology
    from cobel_amd.interface.simulator.offline import OfflineSimulator
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box
    nodes, starts = world_of(c)
    S, n, pick = len(nodes), c['n'], c['pick']
    if c['kind'] == 'graph':    # pose observations; the feature table is the case's own
        env = Topology(nodes, starts, n_envs=n, seed=SEED, instance_base=c['base'])
    else:
        obs = {tuple(nodes[key]['pose']): o for key, o in zip(nodes, np.eye(S))}
        env = Topology(nodes, starts, OfflineSimulator(obs, Box(0.0, 1.0, (S,))), n_envs=n, seed=SEED,
                       instance_base=c['base'])
    ag = MFEC(env.observation_space, env.action_space, EpsilonGreedy(c['eps']), capacity=c['capacity'],
              k=c['k'], projection_size=c['D'], rng=np.random.default_rng(c['seed']))
    if c['kind'] == 'graph':
        ag.feature_table = lambda interface: np.ascontiguousarray(features_of(c, S))
    ag.record_steps, ag.track_instances = c['trials'] * c['steps'], True
    ref, rag, tab = run_reference(c)
    try:
        ag.train(env, c['trials'], c['steps'])
    except NotImplementedError as err:      # two nodes whose few random features are allclose
        assert 'allclose' in str(err), err
        REFUSED.append(c['seed'])
        return [] if ref is None else ['the device refuses a world the restatement accepts']
    if ref is None:
        return ['the device accepts a world the restatement refuses']
    bad = []

    def cmp(name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append(name)

    w = env._tables()
    cmp('next', w['next'], tab['next'])
    cmp('rewards', np.asarray(w['rewards'], dtype=np.float64), tab['reward'])
    cmp('terminals', np.asarray(w['terminals']).astype(np.uint8), tab['terminal'])
    cmp('starts', np.asarray(w['starting_states']), tab['starts'])
    cmp('features', ag.features, features_of(c, S))
    rows = ag.recorded_steps(pick)
    cmp('state', rows[:, 0], ref['state'])
    cmp('action', rows[:, 1], ref['action'])
    cmp('q', rows[:, 4:], ref['q'])
    cmp('latencies', ag.monitors.lat_trace.cpu().numpy()[pick], ref['steps'])
    for a, (b, r) in enumerate(zip(ag.memory(pick).buffers, rag.Q.buffers)):
        cmp('buffer %d ids' % a, b.ids, r.ids)
        cmp('buffer %d values' % a, b.values, r.values)
        cmp('buffer %d times' % a, b.times, r.times)
    got = ag.predict_on_batch(range(S))
    cmp('predict', got if n == 1 else got[pick].cpu().numpy(), ref['predict'])
    return bad


def main() -> int:
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    failed = []
    for seed in range(first, first + count):
        c = draw_case(seed)
        try:
            bad = run_case(c)
        except Exception as e:       # (not a mismatch: nothing more is started on the device)
            print('ERROR %s: %s' % (type(e).__name__, str(e)[:300]), describe(c), flush=True)
            return 2
        if bad:
            failed.append(seed)
        print('MISMATCH %s' % bad[:6] if bad else ('refused' if seed in REFUSED else 'ok'), describe(c),
              flush=True)
    print('cases %d, failing %d: %s; refused (allclose features): %d %s'
          % (count, len(failed), failed, len(REFUSED), REFUSED))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
