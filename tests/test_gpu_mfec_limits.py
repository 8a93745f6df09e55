"""GPU tests of the MFEC kernels at the top of the ranges include/cobel_hip.h documents — 1 024
states, 8 actions, buffers of 2 048 entries, k = 32, 65 536 features — with full buffers, exact ties
and worlds whose rows are distributions, against the NumPy restatement (tests/mfec_common.py, its
helpers for these sizes in tests/mfec_limits_common.py).  Every comparison is np.array_equal; the
calls through the C ABI run on arrays framed by sentinels.  Each test asserts what it set out to
reach (lengths, ties, hits at index 0, replacements, evictions, timed-out and ended trials), so that a
later change of world or seed cannot quietly empty it.

The semantics above 80 entries are the restatement's: the single-leaf rule continued.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfec_common as mc  # noqa: E402
import mfec_limits_common as ml  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xC0BE1
S, A, CAP = 1024, 8, 2048


def lengths_of(k):
    return [k, k + 1, 63, 64, 65, 127, 128, 129, 1000, 2047, 2048]


@pytest.fixture(scope='module')
def torch():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


_TABLES = {}


def tables(kind, n_states=S):
    if (kind, n_states) not in _TABLES:
        _TABLES[kind, n_states] = ml.tables(kind, n_states, seed=4)
    return _TABLES[kind, n_states]


# -- cobel_mfec_estimate on hand-built buffers ---------------------------------------------------------
def estimate_case(kind, k):
    """Two instances of eight buffers whose lengths cover lengths_of(k), at most 64 queried nodes,
    the restatement's answers and what the queries reached."""
    rng = np.random.default_rng(100 * k + len(kind))
    F, tabs = tables(kind)
    lengths = lengths_of(k)
    memories = []
    for i, first in enumerate((0, 3)):
        memories.append([ml.built_buffer(S, n, rng, dups=(0, 30, None)[(i + a) % 3] if n > 40 else 0)
                         for a, n in enumerate(lengths[first:first + A])])
    # the full buffer after its first entry, the oldest, was replaced by a node it did not hold: the
    # copies of the former first node stay behind, the lowest of them answers for that node
    ids = memories[1][A - 1][0]
    assert len(ids) == CAP and (ids == ids[0]).sum() > 1000
    former, ids[0] = int(ids[0]), int(np.setdiff1d(np.arange(S), ids)[-1])
    nodes = [former] + [int(ids[0]) for m in memories for ids, _, _ in m]
    nodes += [int(np.setdiff1d(np.arange(S), ids)[a]) for m in memories for a, (ids, _, _) in enumerate(m)]
    nodes += [int(ids[len(ids) // 2]) for m in memories for ids, _, _ in m]
    nodes += [int(x) for x in rng.integers(0, S, 40)]
    nodes = list(dict.fromkeys(nodes))[:64]
    refs = [ml.load_memory(mc.RefQEC(F, A, CAP, k, tabs), m, 0) for m in memories]
    want = np.zeros((2, len(nodes), A))
    seen = dict(first=0, elsewhere=0, zero=0, knn=0, ties=0, lengths=set(), dup_first=0, dup_later=0)
    for i, Q in enumerate(refs):
        Q.query = ml.tree_query
        for b, s in enumerate(nodes):
            for a, buf in enumerate(Q.buffers):
                want[i, b, a] = Q.estimate(s, a)
                hit = Q.find_state(buf, s)
                if hit is not None:
                    seen['first' if hit == 0 else 'elsewhere'] += 1
                    seen['dup_first'] += hit == 0 and buf.ids.count(buf.ids[0]) >= 20
                    seen['dup_later'] += hit > 0 and buf.ids.count(buf.ids[hit]) >= 20
                    assert want[i, b, a] == buf.values[hit]
                elif len(buf) <= k:
                    seen['zero'] += 1
                else:
                    d = np.sort(tabs[0][s, buf.ids])
                    seen['knn'] += 1
                    seen['ties'] += d[k - 1] == d[k]
                    seen['lengths'].add(len(buf))
    return F, memories, nodes, refs, want, seen


@pytest.mark.parametrize('k', [1, 3, 32])
@pytest.mark.parametrize('kind', ['random', 'lattice', 'onehot'])
def test_estimate_on_built_buffers(torch, kind, k):
    """One launch over two instances x eight actions whose buffer lengths are k, k + 1, 63, 64, 65,
    127, 128, 129, 1 000, 2 047 and 2 048 (32 rounds of the walk), capacity 2 048: nodes held at index
    0 (many of them duplicated tens to a thousand times further on), held elsewhere, and not held.
    ``lattice`` and ``onehot`` tie the k-th with the (k + 1)-th nearest entry: push order and the
    unstable sort decide the sum."""
    F, memories, nodes, refs, want, seen = estimate_case(kind, k)
    print('estimate %s k=%d: %s' % (kind, k, {n: v for n, v in seen.items() if n != 'lengths'}))
    assert seen['lengths'] == {n for n in lengths_of(k) if n > k}, seen['lengths']
    assert seen['first'] >= 16 and seen['dup_first'] >= 4 and seen['elsewhere'] > 0 and seen['dup_later'] >= 1
    assert seen['zero'] > 0 and seen['knn'] >= 100
    # (random rows tie only through the duplicates of a first node; one-hot rows always)
    assert seen['ties'] == seen['knn'] if kind == 'onehot' else seen['ties'] > 0
    dev = ml.DeviceMFEC(torch, F, 2, A, CAP, k)
    for i, m in enumerate(memories):
        dev.load(i, m, 0)
    got = dev.estimate(nodes)
    if not np.array_equal(got, want):
        i, b, a = np.argwhere(got != want)[0]
        raise AssertionError('instance %d node %d action %d (length %d): %r != %r'
                             % (i, nodes[b], a, len(memories[i][a][0]), got[i, b, a], want[i, b, a]))
    dev.check(refs, 'estimate')          # (a read-only call: the memory is as loaded)
    assert not dev.host('clock').any()


# -- cobel_mfec_run at and across capacity -----------------------------------------------------------------
RUN_TRIALS, RUN_STEPS, RUN_EPS, RUN_K, RUN_BASE = 6, 60, 0.3, 3, 40


def run_world():
    nodes, starts = ml.random_graph(S, A, seed=21, goals=48)
    return ml.tables_of(nodes, starts)


def run_memory(case, rng):
    """(memory, clock) preloaded into instance 0."""
    if case == 'crossing':          # a few entries short of capacity: appends, then replacements
        return [ml.built_buffer(S, CAP - 1 - a % 4, rng, dups=CAP - 200) for a in range(A)], CAP
    if case == 'equal_stamps':      # np.argmin takes the FIRST of 2 048 equal stamps
        return [ml.built_buffer(S, CAP, rng, dups=CAP - 200, times=7) for a in range(A)], 7
    if case == 'stamps_ahead':      # nothing is older than the episode: nothing is replaced
        return [ml.built_buffer(S, CAP, rng, dups=CAP - 200, times=10 ** 6) for a in range(A)], 0
    assert case == 'in_place'       # long buffers that hold most nodes at an index above 0
    return [ml.built_buffer(S, 2000, rng) for a in range(A)], 2000


def run_case(case):
    tab = run_world()
    F, tabs = tables('lattice')
    memory, clock = run_memory(case, np.random.default_rng(len(case)))
    out = []
    for i, (m, c) in enumerate(((memory, clock), (None, 0))):
        ag, env, pol = ml.restated(tab, F, tabs, A, RUN_BASE + i, SEED, RUN_EPS, CAP, RUN_K,
                                   memory=m, clock=c)
        counts, tr = ml.count_updates(ag.Q), mc.new_trace()
        ag.train(env, RUN_TRIALS, RUN_STEPS, trace=tr)
        out.append((ag, env, pol, counts, tr))
    return tab, F, memory, clock, out


@pytest.mark.parametrize('case', ['crossing', 'equal_stamps', 'stamps_ahead', 'in_place'])
def test_run_from_a_preloaded_memory(torch, case):
    """cobel_mfec_run through the C ABI on framed arrays, six short trials on the 1 024-node,
    8-action world: instance 0 starts from a preloaded memory (see run_memory), instance 1 next to it
    from an empty one.  Steps and estimates, buffers, len, clock, counters and latencies equal the
    restatement started from the same memory; nothing behind len or outside an array is written."""
    from cobel_amd import _lib
    tab, F, memory, clock, refs = run_case(case)
    counts = refs[0][3]
    print('run %s: %s, bystander %s' % (case, counts, refs[1][3]))
    if case == 'crossing':
        assert counts['append'] >= 8 and counts['replace'] >= 1
    if case == 'equal_stamps':
        assert counts['replace'] >= 8 and counts['append'] == 0
        assert all(b.times[0] > 7 for b in refs[0][0].Q.buffers), 'index 0 goes first'
    if case == 'stamps_ahead':
        assert counts['refused'] >= 8 and counts['replace'] == counts['append'] == 0
    if case == 'in_place':
        moved = sum(int((np.array(b.times[1:2000]) > 2000).sum()) for b in refs[0][0].Q.buffers)
        assert counts['inplace'] >= 8 and moved >= 8 and counts['replace'] == 0
    assert refs[1][3]['append'] > 0 and any(refs[0][4]['ended'])
    dev = ml.DeviceMFEC(torch, F, 2, A, CAP, RUN_K, steps=RUN_STEPS, trace_cap=RUN_TRIALS * RUN_STEPS,
                        trial_cap=RUN_TRIALS)
    dev.load(0, memory, clock)
    dev.set_counters([1, 1], [0, 0])        # (the restated environment's constructor draws a start)
    world = ml.make_world(tab['next'], tab['reward'], tab['terminal'], tab['starts'])
    try:
        dev.run(world, RUN_TRIALS, SEED, RUN_BASE, RUN_EPS)
    finally:
        _lib.check(_lib.lib().cobel_world_destroy(world))
    dev.check([r[0] for r in refs], case)
    inst, lat = dev.host('inst'), dev.host('lat_trace')
    for i, (ag, env, pol, _, tr) in enumerate(refs):
        ml.assert_trace(dev.trace_rows(i), tr, A, '%s instance %d' % (case, i))
        assert np.array_equal(lat[i], tr['steps']), (case, i)
        assert inst[i, _lib.I_CTR_ENV] == env.rng.index == 1 + RUN_TRIALS
        assert inst[i, _lib.I_CTR_POLICY] == pol.rng.index == len(tr['sar'])
        assert inst[i, _lib.I_TRIAL] == RUN_TRIALS


# -- whole sessions through the MFEC class -------------------------------------------------------------------
def class_case(nodes, starts, cfg, F=None, n=1):
    import test_gpu_mfec as tg
    env = tg.make_env(None, nodes=nodes, starts=starts, base=int(cfg[0]), n=n)
    out, ag = tg.device_case(env, cfg, features=F)
    return out, ag, env, tg.tab_of(env)


SESSIONS = {
    # name: (states, actions, goals, features, [instance, trials, steps, capacity, k, test trials, eps x 1e6])
    'top_of_the_range': (1024, 8, 48, 'lattice', [31, 130, 60, 2048, 32, 0, 300000]),
    'seven_actions_evicting': (600, 7, 30, 'random', [32, 90, 60, 40, 5, 0, 300000]),
}


def session_world(name):
    n_states, n_actions, goals, kind, cfg = SESSIONS[name]
    nodes, starts = ml.random_graph(n_states, n_actions, seed=len(name), goals=goals)
    F, tabs = tables(kind, n_states)
    return nodes, starts, F, tabs, cfg


@pytest.mark.parametrize('name', list(SESSIONS))
def test_sessions_at_the_top_of_the_range(name):
    """MFEC.train on random graphs (Topology nodes with eight, or seven, neighbours): 1 024 states,
    8 actions, k = 32 on lattice features until a buffer holds more than 128 entries; 600 states, 7
    actions with a capacity that evicts.  The whole record, predict_on_batch over all nodes included."""
    nodes, starts, F, tabs, cfg = session_world(name)
    out, ag, env, tab = class_case(nodes, starts, cfg, F)
    ref, rag = mc.run_restatement(tab, F, cfg, SEED, tables=tabs, query=ml.tree_query)
    mc.assert_same_record(out, ref, what=name)
    lens = out['buf_len']
    print('%s: longest buffer %d, %d evictions, %d of %d trials ended'
          % (name, lens.max(), rag.Q.evicted, out['ended'].sum(), len(out['ended'])))
    assert (ag.n_states, ag.n_actions) == SESSIONS[name][:2]
    if name == 'top_of_the_range':
        assert lens.max() > 128 and ag.k == 32 and (out['q'] != 0).any()
    else:
        assert rag.Q.evicted >= 10 and lens.max() == cfg[3]


LONG = [39, 10, 2000, 60, 3, 0, 100000]     # one far goal: a random walk of about 45 * 45 steps


def test_trials_of_thousands_of_steps():
    """steps_per_trial = 2 000 on a line of 45 nodes whose only goal is at the far end: trials that
    time out (the episode is dropped) and trials that end (episodes of up to thousands of events are
    written back), the episode scratch at its longest."""
    nodes, starts = ml.line_graph(45)
    out, ag, env, tab = class_case(nodes, starts, LONG)
    ref, rag = mc.run_restatement(tab, ag.features, LONG, SEED, query=ml.tree_query)
    mc.assert_same_record(out, ref, what='long trials')
    ended = out['ended']
    print('long trials: steps %s' % out['steps'].tolist())
    assert ended.any() and not ended.all(), 'both timed-out and ended trials'
    assert out['steps'][ended].max() >= 1000 and (out['steps'][~ended] == LONG[2] - 1).all()


def test_long_trials_in_a_launch_of_65_instances():
    """The same session in a launch of 65 instances: three of them equal their own single-instance
    runs (latencies, buffers, predict_on_batch)."""
    import test_gpu_mfec as tg
    nodes, starts = ml.line_graph(45)
    n, (base, trials, steps, capacity, k, _, eps6) = 65, LONG

    def run(n_envs, first):
        env = tg.make_env(None, nodes=nodes, starts=starts, n=n_envs, base=first)
        ag = tg.make_agent(env, capacity, k, eps6 / 1e6, base, record=0)
        ag.track_instances = True
        ag.train(env, trials, steps)
        return ag, ag.monitors.lat_trace.cpu().numpy()

    ag, lat = run(n, base)
    seen = set()
    for i in (0, 31, 64):
        solo, solo_lat = run(1, base + i)
        assert np.array_equal(solo_lat[0], lat[i]), i
        for a, b in zip(solo.memory(0).buffers, ag.memory(i).buffers):
            for x, y in zip(a, b):
                assert np.array_equal(x, y), i
        assert np.array_equal(solo.predict_on_batch(range(45)), ag.predict_on_batch(range(45))[i].cpu().numpy())
        seen.add(lat[i].tobytes())
    assert len(seen) == 3, 'the instances ran the same stream'
    assert (lat == steps - 1).any() and (lat < steps - 1).any()


# -- cobel_mfec_pairs at its limits ------------------------------------------------------------------------------
def test_pair_tables_of_1024_states(torch):
    """S = 1 024: the S * S index arithmetic and the launch grid of 4 096 blocks."""
    F = ml.features('random', S, seed=9)
    F[5] = F[4]
    F[7] = F[6] * (1 + 9e-5) + 5e-7
    F[1023] = F[1022] * (1 + 2e-4)
    R, same = ml.pair_tables(F)
    r, s = ml.device_pairs(torch, F)
    assert r.intact() and s.intact()
    assert np.array_equal(r.view.cpu().numpy(), R)
    assert np.array_equal(s.view.cpu().numpy().astype(bool), same)
    assert same[4, 5] and same[6, 7] and not same[1022, 1023] and same.sum() == S + 4


def test_pair_tables_of_65536_features(torch):
    """The sequential sum at the longest row the header allows."""
    from cobel_amd import _lib
    D = _lib.MFEC_MAX_FEATURES
    assert D == 65536
    F = np.random.default_rng(8).random((8, D))
    F[3] = F[2] * (1 + 5e-5)
    F[3, D - 1] = F[2, D - 1] * (1 + 3e-4)         # the last feature alone tells the two rows apart
    F[5] = F[4] * (1 + 5e-5)
    R, same = ml.pair_tables(F)
    r, s = ml.device_pairs(torch, F)
    assert r.intact() and s.intact()
    assert np.array_equal(r.view.cpu().numpy(), R)
    assert np.array_equal(s.view.cpu().numpy().astype(bool), same)
    assert not same[2, 3] and same[4, 5] and same.sum() == 8 + 2
    assert not np.array_equal(R, ((F[:, None] - F[None]) ** 2).sum(axis=2)), 'the order of the sum shows'


def test_pair_tables_of_one_hot_rows(torch):
    """S = D = 1 024, np.eye: every off-diagonal distance exactly 2, ``same`` the identity."""
    F, (R, same) = tables('onehot')
    r, s = ml.device_pairs(torch, F)
    assert r.intact() and s.intact()
    assert np.array_equal(r.view.cpu().numpy(), R) and R[0, 1] == 2.0 and R[3, 3] == 0.0
    assert np.array_equal(s.view.cpu().numpy(), np.eye(S, dtype=np.uint8))


# -- a world whose rows are distributions ------------------------------------------------------------------
def test_run_on_a_world_with_distribution_rows(torch):
    """cobel_world_create_n + cobel_world_set_transitions (40 states, 5 actions, up to three
    successors per pair), a training session of cobel_mfec_run in two launches: the successor of every
    step is drawn — one double of the ENV stream (sub-stream 1) per step at the counter the start
    draws (sub-stream 0) share.  The MFEC class runs on a Topology, which has no such rows, so this
    stays at the level of the C ABI."""
    from cobel_amd import _lib
    n_states, n_actions, trials, steps, cap, k, eps, base, N = 40, 5, (12, 30), 25, 20, 3, 0.3, 50, 3
    tab, sas = ml.drawn_world(n_states, n_actions, seed=6)
    F = ml.features('random', n_states, seed=6)
    tabs = ml.pair_tables(F)
    refs = []
    for i in range(N):
        ag, env, pol = ml.restated(tab, F, tabs, n_actions, base + i, SEED, eps, cap, k, drawn=True)
        tr = mc.new_trace()
        ag.train(env, trials[1], steps, trace=tr)
        refs.append((ag, env, pol, tr))
    assert sum(r[0].Q.evicted for r in refs) > 0 and all(any(r[3]['ended']) for r in refs)
    multi = np.count_nonzero(sas, axis=2) > 1
    drawn = sum(int(multi[int(s), int(a)]) for r in refs for s, a, _, _ in r[3]['sar'])
    assert drawn >= 100, 'steps whose successor had to be drawn'
    dev = ml.DeviceMFEC(torch, F, N, n_actions, cap, k, steps=steps, trace_cap=trials[1] * steps,
                        trial_cap=trials[1])
    dev.set_counters([1] * N, [0] * N)
    world = ml.make_world(tab['next'], tab['reward'], tab['terminal'], tab['starts'], sas=sas)
    try:
        for target in trials:
            dev.run(world, target, SEED, base, eps)
            assert (dev.host('inst')[:, _lib.I_TRIAL] == target).all()
    finally:
        _lib.check(_lib.lib().cobel_world_destroy(world))
    dev.check([r[0] for r in refs], 'drawn')
    inst, lat = dev.host('inst'), dev.host('lat_trace')
    for i, (ag, env, pol, tr) in enumerate(refs):
        ml.assert_trace(dev.trace_rows(i), tr, n_actions, 'drawn instance %d' % i)
        assert np.array_equal(lat[i], tr['steps']), i
        # one per reset (the constructor's included) plus one per step
        assert inst[i, _lib.I_CTR_ENV] == env.rng.index == 1 + trials[1] + len(tr['sar'])
        assert inst[i, _lib.I_CTR_POLICY] == pol.rng.index == len(tr['sar'])
