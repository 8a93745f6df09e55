"""GPU tests of PMA's per-instance parameter sets (``cobel_pma_mem_sets_t.param_index`` in
cobel_pma_trial, cobel_pma_replay, cobel_pma_store, cobel_pma_update_sr, cobel_pma_gain_batch,
cobel_pma_gain_seq and cobel_pma_update_q_sets, through PMA / PMAMemory with array-valued
attributes): one launch with sets against the scalar launches of the same global instances in
every kernel form, seven instances in one set against the scalar launch, instance by instance
against the NumPy restatement run with each instance's own ten values, the memory's own calls, and
a sweep under ``GridSearchOptimizer.fit_vectorised``.

Seven instances from global instance 5; the set of instance i is ``WHICH7[i]`` (three sets that
differ in every value, duplicates, not contiguous).  Bar as in test_gpu_pma.py: float64, everything
compared is equal bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

import pma_common as pc
import pma_sets_common as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'


def groups(which):
    """Contiguous runs of one set: (first instance, count, set)."""
    out = []
    for i, s in enumerate(which):
        if out and out[-1][2] == s:
            out[-1][1] += 1
        else:
            out.append([i, 1, s])
    return [tuple(g) for g in out]


@functools.lru_cache(maxsize=None)
def sets_run(name, shared, need):
    """The launch with sets of a case (host arrays only; shared between the tests, read-only)."""
    got, (env, agent, mem) = sc.run(name, sc.N, sc.BASE, sc.columns(sc.SETS3, sc.WHICH7), shared,
                                    need)
    assert mem._psets['agent']['n'] == 3
    # (np.unique sorts the rows — by learning_rate first, 0.5 < 0.75 < 0.9 — so set k of the table
    #  is SETS3[(1, 2, 0)[k]])
    index = mem._psets['agent']['index'].cpu().numpy().view(np.uint16).tolist()
    assert [(1, 2, 0)[k] for k in index] == list(sc.WHICH7)
    return got


def scalar_runs_equal(name, shared, need, got):
    """Every contiguous run of one set as a scalar launch of its own on the same global
    instances."""
    for first, count, s in groups(sc.WHICH7):
        want, (_, _, mem) = sc.run(name, count, sc.BASE + first, sc.SETS3[s], shared, need)
        assert mem._psets == {} and mem._held is None
        part = {k: (v[:, first:first + count] if k == 'replays' else v[first:first + count])
                for k, v in got.items()}
        sc.assert_rows_equal(part, want, slice(None), (name, first, s))


# ---------------------------------------------------------------------------------------------
# 1. one launch with sets equals the scalar launches of the same global instances
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('need', ['host', 'device'])
@pytest.mark.parametrize('shared', [False, True], ids=['own_policy', 'shared_policy'])
@pytest.mark.parametrize('name', list(sc.WORLDS))
def test_one_launch_with_sets_equals_the_scalar_launches(name, shared, need):
    """Q, rewards, states, terminals, T, SR, update_mask, the counters, ``inst``, the latency
    trace, ``last`` and the start and end replay records.  small_3x4: S x A = 48, less than a
    wavefront; demo_5x5: 100, two passes; eight_18x8: the eight-action loops; wide_17x16: the wide
    form, ``update_sr`` by the blocked kernels with a gamma per instance and, with the need on the
    device, the wide need solve with three workspaces for seven instances — a batch of it
    crosses set boundaries."""
    got = sets_run(name, shared, need)
    trials, _, batch = sc.session_of(name)
    assert got['replays'].shape == (2 * trials, sc.N, batch, 5)
    from cobel_amd import _lib
    assert (got['inst'][:, _lib.I_TRIAL] == trials).all()
    scalar_runs_equal(name, shared, need, got)
    # instances of one set differ by their streams, instances of different sets by their sets too
    assert not np.array_equal(got['Q'][0], got['Q'][3])
    assert not np.array_equal(got['SR'][0], got['SR'][1])


def test_one_launch_with_sets_equals_the_scalar_launches_blocked_sr(monkeypatch):
    """The small world with ``update_sr`` forced through the blocked kernels, which take gamma per
    instance; the result equals the LDS kernel's launch with sets as well."""
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PMA_SR', 'blocked')
    got, _ = sc.run('small_3x4', sc.N, sc.BASE, sc.columns(sc.SETS3, sc.WHICH7))
    scalar_runs_equal('small_3x4', False, 'host', got)
    monkeypatch.delenv('COBEL_DEBUG_PMA_SR')
    monkeypatch.delenv('COBEL_DEBUG')
    sc.assert_rows_equal(got, sets_run('small_3x4', False, 'host'), slice(None), 'lds')


# ---------------------------------------------------------------------------------------------
# 2. seven instances in ONE set
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True], ids=['own_policy', 'shared_policy'])
@pytest.mark.parametrize('name', ['small_3x4', 'eight_18x8'])
def test_seven_instances_in_one_set_equal_the_scalar_launch(name, shared):
    got, (_, _, mem) = sc.run(name, sc.N, sc.BASE, sc.columns(sc.SETS3[1:], sc.ONE7), shared)
    assert mem._psets['agent']['n'] == 1
    assert not mem._psets['agent']['index'].cpu().numpy().any()
    want, (_, _, plain) = sc.run(name, sc.N, sc.BASE, sc.SETS3[1], shared)
    assert plain._psets == {}
    assert got.keys() == want.keys()
    for key in want:
        assert got[key].dtype == want[key].dtype, key
        assert got[key].tobytes() == want[key].tobytes(), key


# ---------------------------------------------------------------------------------------------
# 3. against the restatement, instance by instance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shared', [False, True], ids=['own_policy', 'shared_policy'])
@pytest.mark.parametrize('name', sc.REF_WORLDS)
def test_sets_equal_the_restatement_instance_by_instance(name, shared):
    """Every instance against ``RefPMA`` / ``RefPMAMemory(sr_by_elimination=True)`` built with its
    own ten values; nothing injected: the device runs its own ``update_sr``, the restatement the
    same elimination (as scripts/fuzz_pma.py compares scalar launches)."""
    got = sets_run(name, shared, 'host')
    for i, s in enumerate(sc.WHICH7):
        tr, agent, mem, index = sc.ref_run(name, sc.BASE + i, s, shared)
        what = (name, i, s)
        assert np.array_equal(got['lat_trace'][i], tr['steps']), what
        assert np.array_equal(got['last'][i], tr['last'][-1]), what
        assert np.array_equal(got['replays'][0::2, i], np.array(tr['replay_start'])), what
        assert np.array_equal(got['replays'][1::2, i], np.array(tr['replay_end'])), what
        assert np.array_equal(got['Q'][i], agent.Q), what
        for key in ('T', 'SR', 'rewards', 'states', 'terminals'):
            assert np.array_equal(got[key][i], getattr(mem, key)), what + (key,)
        assert np.array_equal(got['update_mask'][i].astype(bool), mem.update_mask), what
        pol = got['act_ctr'][i] if shared else got['pol_ctr'][i]
        assert [got['env_ctr'][i], got['act_ctr'][i], got['mem_ctr'][i], pol] == index, what


# ---------------------------------------------------------------------------------------------
# 4. the memory's own calls
# ---------------------------------------------------------------------------------------------
def memory_of(name, params):
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    _, _, sas, wide = sc.world_of(name)
    mem = PMAMemory(sas, EpsilonGreedy(params['memory_epsilon']),
                    learning_rate=params['learning_rate'], learning_rate_q=params['learning_rate_q'],
                    gamma=params['gamma'], gamma_q=params['gamma_q'], wide=wide)
    mem.learning_rate_T, mem.min_gain = params['learning_rate_T'], params['min_gain']
    mem.bind(sc.N, seed=sc.SEED, instance_base=sc.BASE)
    return mem


def memory_script(name, mem) -> dict:
    """store, replay (1, 7 and 40 rounds: the last beyond the 34 rows a power table starts with),
    update_sr, compute_gain_batch, compute_gain (7 steps and 256, the top of PMA_MAX_SEQ),
    update_q — and the counters at rest where they must be."""
    import torch
    _, tabs, sas, _ = sc.world_of(name)
    n, S, A = sc.N, sas.shape[0], sas.shape[1]
    out = {'SR0': np.asarray(mem.SR)}
    rows = pc.walk_stores(tabs, 40, seed=3)
    for k in range(len(rows)):              # instance i sees the walk i experiences late
        pick = [rows[max(k - i, 0)] for i in range(n)]
        mem.store({'state': [r[0] for r in pick], 'action': [r[1] for r in pick],
                   'reward': [r[2] for r in pick], 'next_state': [r[3] for r in pick],
                   'terminal': [r[4] for r in pick]})
    counters = lambda: (mem.counter.clone(), mem._policy_counter().clone())   # noqa: E731
    at_rest = counters()
    assert not at_rest[0].any() and not at_rest[1].any()
    start = int(tabs['starts'][0])
    q = sc.q_start(name)
    for length in (1, 7):
        ups, q = mem.replay(q, None, length, start)
        out['replay_%d' % length] = np.array([pc.rows_of(u) for u in ups])
    mem.update_sr()
    ups, q = mem.replay(q, pc.masked_actions(tabs) if A == 4 else None, 40, rows[-1][3])
    out['replay_40'] = np.array([pc.rows_of(u) for u in ups])
    out['Q'] = q.cpu().numpy()
    moved = counters()
    assert (moved[0] >= 48).all()
    out['mem_ctr'], out['pol_ctr'] = moved[0].cpu().numpy(), moved[1].cpu().numpy()
    out['gain_batch'] = mem.compute_gain_batch(q, None).cpu().numpy()
    walk = pc.walk_stores(tabs, 256, seed=5)
    keys = ('state', 'action', 'reward', 'next_state', 'terminal')
    seq = lambda rs: [dict(zip(keys, (int(r[0]), int(r[1]), float(r[2]), int(r[3]), int(r[4]))))  # noqa: E731
                      for r in rs]
    out['gain_seq'] = mem.compute_gain(q, None, [seq(walk[:7]), seq(walk)]).cpu().numpy()
    update = [dict(e, terminal=1) for e in seq(walk[:5])]
    q2 = q.clone()
    assert mem.update_q(q2, update) is q2
    out['update_q'] = q2.cpu().numpy()
    assert not np.array_equal(out['update_q'], out['Q'])
    torch.cuda.synchronize()
    for a, b in zip(moved, counters()):
        assert torch.equal(a, b), 'a gain map, a sequence gain or update_q moved a counter'
    for key in ('rewards', 'states', 'terminals', 'T', 'SR', 'update_mask'):
        out[key] = mem._dev[key].cpu().numpy()
    return out


@pytest.mark.parametrize('name', ['demo_5x5', 'eight_18x8', 'wide_17x16'])
def test_memory_calls_use_the_parameters_of_each_instance(name):
    mem = memory_of(name, sc.columns(sc.SETS3, sc.WHICH7))
    got = memory_script(name, mem)
    held = mem._psets['memory']
    assert held['n'] == 3 and held['gamma_pow'].shape == (3, 257)
    assert got['SR0'].shape[0] == sc.N          # the constructor's gammas: an SR per instance
    for s in range(3):
        plain = memory_of(name, sc.SETS3[s])
        want = memory_script(name, plain)
        assert plain._psets == {}
        rows = [i for i, w in enumerate(sc.WHICH7) if w == s]
        for key in want:
            w = want[key] if key != 'SR0' else np.broadcast_to(want[key], got[key].shape)
            assert got[key].shape == w.shape, (s, key)
            assert np.array_equal(got[key][rows], w[rows]), (s, key)
    assert not np.array_equal(got['gain_batch'][0], got['gain_batch'][1])
    assert not np.array_equal(got['update_q'][0], got['update_q'][1])


def test_update_q_of_the_agent_uses_the_parameters_of_each_instance():
    """``PMA.update_q`` after a session: ``cobel_pma_update_q_sets`` with the agent's learning rate
    and ``gamma ** k`` of every instance's set, against the scalar call per run of one set."""
    name = 'demo_5x5'
    update = [{'state': 12, 'action': 1, 'reward': 0.5, 'next_state': 7, 'terminal': 1},
              {'state': 7, 'action': 2, 'reward': 0.0, 'next_state': 8, 'terminal': 1},
              {'state': 8, 'action': 1, 'reward': 10.0, 'next_state': 3, 'terminal': 1}]

    def after(n, base, params):
        env, agent, mem = sc.build(name, n, base, params)
        agent.train(env, 1, 10, 4)
        before = agent._q.cpu().numpy().copy()
        agent.update_q(update)
        return before, agent._q.cpu().numpy()
    before, got = after(sc.N, sc.BASE, sc.columns(sc.SETS3, sc.WHICH7))
    assert not np.array_equal(before, got)
    for first, count, s in groups(sc.WHICH7):
        _, want = after(count, sc.BASE + first, sc.SETS3[s])
        assert np.array_equal(got[first:first + count], want), (first, s)


def test_the_trial_and_the_memory_calls_refuse_bad_sets_before_any_launch():
    """A real launch with its table of sets taken away behind ``_fill_params``: cobel_pma_trial
    (whose refusal needs a world, so a device) and the memory's calls raise, nothing is written."""
    import torch
    env, agent, mem = sc.build('small_3x4', sc.N, sc.BASE, sc.columns(sc.SETS3, sc.WHICH7))
    agent.train(env, 1, 10, 4)
    torch.cuda.synchronize()
    tensors = lambda: [agent._q, mem.counter, mem.policy.counter] + list(mem._dev.values())  # noqa: E731
    before = [t.clone() for t in tensors()]
    fill = type(mem)._fill_params

    def tampered(x, length=0, agent=None):
        held = fill(mem, x, length, agent)
        x.param_sets = None
        return held
    mem._fill_params = tampered
    text = '%s: param_index given without parameter sets'
    with pytest.raises(AssertionError, match=text % 'cobel_pma_trial'):
        agent.train(env, 1, 10, 4)
    with pytest.raises(AssertionError, match=text % 'cobel_pma_update_sr'):
        mem.update_sr()
    with pytest.raises(AssertionError, match=text % 'cobel_pma_replay'):
        mem.replay(agent._q, None, 4, 8)
    with pytest.raises(AssertionError, match=text % 'cobel_pma_store'):
        mem.store({'state': 1, 'action': 0, 'reward': 1.0, 'next_state': 2, 'terminal': 1})
    torch.cuda.synchronize()
    for a, b in zip(before, tensors()):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
# 6. fit_vectorised through the sweep demo
# ---------------------------------------------------------------------------------------------
def test_fit_vectorised_equals_fit_combination_by_combination(tmp_path):
    """scripts/demo_pma_sweep.py: 4 combinations x 3 runs on the instance axis of one session
    against ``fit``, which runs the combinations one after the other on the same global
    instances."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import demo_pma_sweep as demo
    from cobel_amd.optimizer import GridSearchOptimizer
    grid = {'learning_rate_q': [0.5, 0.9], 'gamma': [0.8, 0.9]}
    runs = 3
    task = demo.make_task(trials=3, steps=30, batch=8, seed=sc.SEED)
    kept = {}

    def keep(sim, data):
        kept[len(kept)] = np.array(sim['demo'])
        return demo.loss(sim, data)
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    opt = GridSearchOptimizer(str(tmp_path / 'a') + '/', grid, nb_runs=runs)
    fit_v = opt.fit_vectorised(demo.simulation_batch, {'demo': task}, {'demo': None}, keep)
    vectorised, kept = dict(kept), {}
    calls = [0]

    def simulation(task, params):         # run r of combination k is global instance k * runs + r
        lat = demo.simulate(task, params, 1, calls[0])
        calls[0] += 1
        return lat[0]
    opt = GridSearchOptimizer(str(tmp_path / 'b') + '/', grid, nb_runs=runs)
    fit_s = opt.fit(simulation, {'demo': task}, {'demo': None}, keep)
    assert calls[0] == 4 * runs and len(fit_v) == 4
    assert fit_v == fit_s
    for k in range(4):
        assert vectorised[k].shape == (runs, 3)
        assert np.array_equal(vectorised[k], kept[k]), k
    assert len({v.tobytes() for v in vectorised.values()}) > 1
