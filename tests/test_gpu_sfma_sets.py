"""GPU tests of SFMA's per-instance parameter sets (cobel_sfma_run, cobel_sfma_store and
cobel_sfma_replay with ``param_index``, through SFMA / SFMAMemory with array-valued attributes):
one launch with sets against the scalar launches of the same global instances in every kernel
form, identical sets against the scalar launch (the plain-training kernel included), instance by
instance against the NumPy restatement run with each instance's own parameters, the memory's own
calls, per-instance modes, the refusals of the entry points and sentinel frames around the tables.

Bar as in test_gpu_sfma.py: everything compared is bit-equal."""
import numpy as np
import pytest

import frames_common as fc
import sfma_memory_common as mc
import sfma_sets_common as sc
import test_gpu_sfma as ts
from conftest import SEED
from oracle.philox import STREAM_MEMORY, TapeRNG

pytestmark = pytest.mark.gpu

MEMORY_ATTRS = sc.MEMORY


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'


def build(tab, D, n, base, params, opts=None, **force):
    """Agent and environment of ``n`` instances from ``base`` with ``params``: name -> scalar or
    [n] array for the fourteen parameters, ``mode`` -> a name or a list of n names."""
    opts = dict(opts or {}, mode='default')
    env, agent = ts.build(tab, D, opts, n, base, eps=params['epsilon'])
    agent.learning_rate, agent.gamma = params['alpha'], params['gamma']
    agent.M.learning_rate = params['model_lr']
    for k in MEMORY_ATTRS:
        setattr(agent.M, k, params[k])
    agent.M.mode = params['mode']
    for k, v in force.items():
        setattr(agent, k, v)
    return env, agent


def state_of(env, agent):
    """Everything a session leaves behind, as host arrays: tables, model records, counters,
    monitors, the |TD| sums."""
    import torch
    torch.cuda.synchronize()
    out = {'Q': agent._q, 'model': agent.M.table, 'C': agent.M.strength, 'stamp': agent.M.stamp,
           'inst': agent.inst, 'sfma_inst': agent.M.state, 'mem_ctr': agent.M.counter,
           'env_ctr': env.env_ctr, 'pol_ctr': agent.policy.counter,
           'lat_trace': agent.monitors.lat_trace}
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['T'] = np.asarray(agent.M.T).reshape(out['C'].shape)
    out['td'] = np.asarray(agent.td, dtype=np.float64).reshape(-1)
    return out


# ---------------------------------------------------------------------------------------------
# 1. one launch with sets equals the scalar launches
# ---------------------------------------------------------------------------------------------
FORMS = [
    # id, h, w, forcing, expected (form, threads per instance)
    ('k_sfma_2', 5, 5, {}, (0, 64)),
    ('k_sfma_4', 6, 7, {}, (0, 64)),
    ('k_sfma_8', 10, 10, {}, (0, 64)),
    ('one_wave_general', 6, 7, {'force_general_kernel': True}, (0, 64)),
    ('k_sfma_wg', 15, 15, {}, (0, 256)),
    ('streaming', 6, 7, {'force_stream_kernel': True}, (1, 256)),
]


@pytest.mark.parametrize('form', FORMS, ids=[f[0] for f in FORMS])
def test_one_launch_with_sets_equals_the_scalar_launches(form):
    _, h, w, force, plan = form
    _, tab, D, _ = sc.world_of(h, w, 'Euclidean')
    opts = dict(reward_mod_local=True, noreplay_trials=1, test_trials=1)
    trials, steps, B = 3, 30, 10
    total = trials + 2
    env, agent = build(tab, D, 12, sc.BASE, sc.columns(sc.SETS4, sc.WHICH12), opts, **force)
    ts.run_schedule(env, agent, opts, trials, steps, B)
    assert (agent.launch_plan[0], agent.launch_plan[2]) == plan
    assert agent.M._psets['agent']['n'] == 4
    got = state_of(env, agent)
    replayed = 0
    for k in range(4):
        env1, one = build(tab, D, 3, sc.BASE + 3 * k, sc.SETS4[k], opts, **force)
        ts.run_schedule(env1, one, opts, trials, steps, B)
        assert one.M._psets == {} and tuple(one.launch_plan) == tuple(agent.launch_plan)
        want = state_of(env1, one)
        for key in want:
            g = got[key][3 * k:3 * k + 3]
            if key == 'lat_trace':
                g, want[key] = g[:, :total], want[key][:, :total]
            assert g.tobytes() == want[key].tobytes(), (k, key)
        for j in range(3):
            ev = ts.events_of(agent, 3 * k + j)
            assert np.array_equal(ev, ts.events_of(one, j)), (k, j)
            replayed += len(ev)
    assert replayed > 12 * trials * B // 2 and int(agent.replays_done) == replayed


# ---------------------------------------------------------------------------------------------
# 2. identical sets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fast', [True, False], ids=['fast_eligible', 'traced'])
def test_identical_sets_equal_the_scalar_launch(fast):
    """N identical rows are one set; the launch equals the scalar launch bit for bit — on a
    fast-eligible configuration (5x5, plain training, no traces) the run the plain-training kernel
    makes, which a launch with an index does not take."""
    import torch
    _, tab, D, _ = sc.world_of(5, 5, 'DR')
    n, p = 40, sc.SETS8[0]
    assert p['decay_strength'] == 1.0 and 0 <= p['beta'] <= 700 and p['R_threshold'] >= 0
    runs = []
    for sets in (False, True):
        params = dict(p)
        if sets:
            params.update({k: np.full(n, p[k]) for k in sc.PARAMETERS})
            params['mode'] = [p['mode']] * n
        env, agent = build(tab, D, n, 300, params)
        agent.track_instances = agent.keep_replay_trace = not fast
        agent.train(env, 5, 30, 12)
        torch.cuda.synchronize()
        runs.append((env, agent))
    (e1, a), (e2, b) = runs
    assert a.M._psets == {} and b.M._psets['agent']['n'] == 1
    for x, y in ((a._q, b._q), (a.M.strength, b.M.strength), (a.M.table, b.M.table),
                 (a.M.stamp, b.M.stamp), (a.inst, b.inst), (a.M.state, b.M.state),
                 (e1.state, e2.state), (a.M.counter, b.M.counter),
                 (a.monitors.lat_sum, b.monitors.lat_sum), (a.monitors.lat_cnt, b.monitors.lat_cnt),
                 (a.monitors.reward_sum, b.monitors.reward_sum)):
        assert fc.same_bits(x, y)
    assert int(a.replays_done) == int(b.replays_done) > 0
    if not fast:
        for i in (0, n - 1):
            assert np.array_equal(ts.events_of(a, i), ts.events_of(b, i))


# ---------------------------------------------------------------------------------------------
# 3. against the restatement, instance by instance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.ORACLE_CASES))
def test_sets_vs_oracle_instance_by_instance(name):
    """16 instances, 8 sets that vary all fourteen parameters and the mode; train, a no-replay
    train and test; six instances re-run by the restatement with their own parameters."""
    c = sc.ORACLE_CASES[name]
    _, tab, D, _ = sc.world_of(c['h'], c['w'], c['metric'])
    opts = sc.ORACLE_OPTS
    env, agent = build(tab, D, 16, sc.BASE, sc.columns(sc.SETS8, sc.WHICH16), opts)
    ts.run_schedule(env, agent, opts, sc.ORACLE_TRIALS, c['steps'], c['B'])
    assert agent.M._psets['agent']['n'] == 8
    total = sc.ORACLE_TRIALS + opts['noreplay_trials'] + opts['test_trials']
    assert agent.M.modes == [sc.SETS8[s]['mode'] for s in sc.WHICH16]
    for i in c['rerun']:
        ag = sc.oracle_case_run(name, i)
        assert np.array_equal(agent.monitors.lat_trace[i].cpu().numpy()[:total], ag.steps), i
        rp = np.array(ag.replayed, dtype=np.float64).reshape(-1, 8)
        assert len(rp) > 0
        ts.check_events(ts.events_of(agent, i), rp)
        assert np.array_equal(agent.Q[i].cpu().numpy(), ag.Q), i
        assert np.array_equal(agent.M.rewards[i], ag.M.rewards), i
        assert np.array_equal(agent.M.states[i], ag.M.states), i
        assert np.array_equal(agent.M.C[i], ag.M.C), i
        assert np.array_equal(agent.M.T[i], ag.M.T), i
        assert agent.td[i] == float(ag.td), i


# ---------------------------------------------------------------------------------------------
# 4. the memory's own calls
# ---------------------------------------------------------------------------------------------
MEM_COLUMNS = dict(
    decay_inhibition=[0.9, 0.5, 0.8, 0.99, 0.9],
    decay_strength=[1.0, 0.97, 0.9, 1.0, 1.0],
    beta=[20.0, 5.0, 9.0, 40.0, 20.0],
    C_step=[1.0, 0.5, 2.0, 1.0, 1.0],
    I_step=[1.0, 0.3, 0.6, 1.0, 1.0],
    mode=['default', 'reverse', 'blend_forward', 'interpolate', 'default'])


@pytest.mark.parametrize('stream', [False, True], ids=['lds_resident', 'streaming'])
def test_memory_calls_use_the_parameters_of_each_instance(stream):
    import copy
    from cobel_amd import _lib
    from cobel_amd.memory import SFMAMemory
    from cobel_amd.memory.utils import Euclidean
    from test_gpu_sfma_memory import _stores, counter_of
    h, w, n, base, count, L, K = 6, 7, 5, 60, 60, 10, 3
    S, D = h * w, Euclidean(w, h).D
    mem = SFMAMemory(D, S, 4)
    for k, v in MEM_COLUMNS.items():
        setattr(mem, k, v if k == 'mode' else np.array(v))
    mem.launch_flags = _lib.F_SFMA_STREAM if stream else 0
    mem.bind(n, seed=SEED, instance_base=base)
    assert mem.launch_plan()[0] == int(stream)
    refs = []
    for i in range(n):
        ref = mc.RefMemory(D, S, 4, TapeRNG(SEED, base + i, STREAM_MEMORY, double_sub=1),
                           dtype=np.float32)
        for k, v in MEM_COLUMNS.items():
            setattr(ref, k, v[i])
        refs.append(ref)
    assert mem.modes == MEM_COLUMNS['mode']

    def compare(what):
        for i, ref in enumerate(refs):
            assert np.array_equal(mem.C[i], ref.C), (what, i)
            assert np.array_equal(mem.T[i], ref.T), (what, i)
            assert np.array_equal(mem.I[i], ref.I), (what, i)
            assert counter_of(mem, i) == ref.rng.index, (what, i)

    seen = []

    def replays(state, action):
        got = mem.replay(L, state, action)
        for i, ref in enumerate(refs):
            st = None if state is None else int(np.broadcast_to(state, (n,))[i])
            ac = None if action is None else int(np.broadcast_to(action, (n,))[i])
            want = ref.replay(L, st, ac)
            assert mc.DictMemory._rows(got[i]) == [[float(x) for x in e] for e in want], \
                (state, action, i)
            seen.append(len(want))
        compare((state, action))

    s, a, r, ns, nt, _ = _stores(S, n, count, seed=11)
    for k in range(count):
        mem.store({'state': s[k], 'action': a[k], 'reward': r[k], 'next_state': ns[k],
                   'terminal': nt[k]})
        for i, ref in enumerate(refs):
            ref.store(int(s[k, i]), int(a[k, i]), float(r[k, i]), int(ns[k, i]), int(nt[k, i]))
    assert mem._psets['memory']['n'] == 4           # instances 0 and 4 share a set
    compare('stores')
    replays(s[0], None)            # the state given
    replays(None, None)            # drawn
    replays(s[3], a[3])            # the action given
    assert max(seen) == L and sum(seen) > 2 * n * L
    # instances 0 and 4 have one set and differ by their streams only; 0 and 1 differ by their sets
    assert not np.array_equal(mem.C[0], mem.C[1])
    # replay_batch: K replays side by side, each against a copy of the restatement at its place
    c0 = [counter_of(mem, i) for i in range(n)]
    out = mem.replay_batch(K, L, s[5])
    for i, ref in enumerate(refs):
        assert counter_of(mem, i) == c0[i] + K * (L + 2)
        for k in range(K):
            cp = copy.deepcopy(ref)
            cp.rng = TapeRNG(SEED, base + i, STREAM_MEMORY, start=c0[i] + k * (L + 2), double_sub=1)
            want = cp.replay(L, int(s[5, i]))
            m = int(out['length'][i, k])
            assert m == len(want) > 0
            got = [[float(out[key][i, k, j]) for key in
                    ('state', 'action', 'reward', 'next_state', 'terminal')] for j in range(m)]
            assert got == [[float(x) for x in e] for e in want], (i, k)
            if k == 0:
                assert np.array_equal(mem.I[i], cp.I), i
        assert np.array_equal(mem.C[i], ref.C) and np.array_equal(mem.T[i], ref.T), i


# ---------------------------------------------------------------------------------------------
# 5. modes
# ---------------------------------------------------------------------------------------------
def test_modes_per_instance_one_for_all_and_dynamic():
    from cobel_amd import _lib
    from cobel_amd.memory import _device
    _, tab, D, _ = sc.world_of(5, 5, 'DR')
    n = 7
    modes = list(_lib.SFMA_MODES)
    assert len(modes) == n
    env, agent = build(tab, D, n, 40, dict(sc.SETS8[0], mode=modes))
    agent.train(env, 2, 20, 8)
    assert agent.M.modes == modes
    assert [int(m) for m in agent.M.state[:, _lib.SI_MODE].cpu()] == list(range(n))
    agent.M.mode = 'sweeping'                 # a string still sets all instances
    agent.train(env, 1, 20, 8)
    assert agent.M.modes == ['sweeping'] * n
    agent.M.mode = np.array(modes[::-1])      # an array of names, as spread_over_instances gives
    agent.train(env, 1, 20, 8)
    assert agent.M.modes == modes[::-1]
    agent.dynamic = True                      # dynamic mode goes on overriding it
    agent.train(env, 3, 20, 8)
    assert set(agent.M.modes) <= {'default', 'reverse'}
    agent.dynamic = False
    agent.M.mode = modes[:3]                  # a wrong length
    with pytest.raises(AssertionError) as e:
        agent.train(env, 1, 20, 8)
    assert str(e.value) == _device.PER_INSTANCE_SHAPE


# ---------------------------------------------------------------------------------------------
# 6. what the entry points refuse
# ---------------------------------------------------------------------------------------------
def _tamper(mem, change):
    fill = type(mem)._fill_params

    def tampered(struct, agent=None):
        sf = fill(mem, struct, agent)
        change(struct)
        return sf
    mem._fill_params = tampered


def _snapshot(agent):
    # (not `inst`: the head of a session writes the environment's state into it on the host)
    return [t.clone() for t in (agent._q, agent.M.strength, agent.M.table, agent.M.stamp,
                                agent.M.state, agent.M.counter, agent.replays_done)]


REFUSALS = [
    ('index_without_sets', lambda s: setattr(s, 'param_sets', None), AssertionError),
    ('no_sets', lambda s: setattr(s, 'n_param_sets', 0), IndexError),
    ('too_many_sets', lambda s: setattr(s, 'n_param_sets', 65536), IndexError),
    ('sets_misaligned', lambda s: setattr(s, 'param_sets', s.param_sets + 8), AssertionError),
    ('index_misaligned', lambda s: setattr(s, 'param_index', s.param_index + 1), AssertionError),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_the_entry_points_refuse_bad_sets_before_any_launch(case):
    import torch
    _, change, error = case
    _, tab, D, _ = sc.world_of(5, 5, 'DR')
    env, agent = build(tab, D, 12, sc.BASE, sc.columns(sc.SETS4, sc.WHICH12))
    agent.train(env, 1, 20, 8)
    before = _snapshot(agent)
    _tamper(agent.M, change)
    with pytest.raises(error):
        agent.train(env, 1, 20, 8)                                       # cobel_sfma_run
    with pytest.raises(error):
        agent.M.replay(6, 3)                                             # cobel_sfma_replay
    with pytest.raises(error):
        agent.M.store({'state': 3, 'action': 1, 'reward': 0.0, 'next_state': 4, 'terminal': 1})
    torch.cuda.synchronize()
    for x, y in zip(before, _snapshot(agent)):
        assert fc.same_bits(x, y)


def test_no_instances_with_sets_is_a_no_op():
    import ctypes as C
    import torch
    from cobel_amd import _lib
    _, tab, D, _ = sc.world_of(5, 5, 'DR')
    env, agent = build(tab, D, 12, sc.BASE, sc.columns(sc.SETS4, sc.WHICH12))
    agent.train(env, 1, 20, 8)
    before = _snapshot(agent)
    m, dev = agent.M._mem()
    assert m.param_index and m.n_param_sets == 4
    m.n = 0
    _lib.check(_lib.lib().cobel_sfma_store(C.byref(m), _lib.ptr(agent.M.strength),
                                           _lib.current_stream(dev)))
    _tamper(agent.M, lambda s: setattr(s, 'n', 0))
    agent.train(env, 1, 20, 8)
    torch.cuda.synchronize()
    for x, y in zip(before, _snapshot(agent)):
        assert fc.same_bits(x, y)


# ---------------------------------------------------------------------------------------------
# 7. sentinel frames around the set table and the index
# ---------------------------------------------------------------------------------------------
def test_set_table_and_index_inside_sentinel_frames():
    """One launch of cobel_sfma_run and one of cobel_sfma_replay with the sets and the index inside
    guards: no guard byte changes, the tables themselves are unchanged, and the run equals the
    unframed one bit for bit (the guards hold zeros: a read past the index would pick set 0, one
    past the sets a set of zeros)."""
    _, tab, D, _ = sc.world_of(6, 7, 'Euclidean')
    cols = sc.columns(sc.SETS4, sc.WHICH12[::-1])       # (the last instances are not set 0's)
    results = []
    for framed in (False, True):
        env, agent = build(tab, D, 12, sc.BASE, cols)
        agent.train(env, 2, 25, 8)                      # builds the agent's table of sets
        agent.M.replay(6, 3)                            # ... and the memory's
        frames, kept = fc.Frames(), {}
        if framed:
            for who in ('agent', 'memory'):
                held = agent.M._psets[who]
                for key in ('sets', 'index'):
                    kept[who, key] = held[key].clone()
                    frames.swap(held, key, 0)
        agent.train(env, 2, 25, 8)                      # cobel_sfma_run
        replayed = agent.M.replay(8, 5)                 # cobel_sfma_replay
        if framed:
            frames.check()
            for (who, key), t in kept.items():
                assert fc.same_bits(agent.M._psets[who][key], t), (who, key)
        out = state_of(env, agent)
        out['replayed'] = np.array([mc.DictMemory._rows(r) for r in replayed if len(r) == 8])
        out['I'] = np.asarray(agent.M.I)
        results.append(out)
    assert len(results[0]['replayed']) > 0
    fc.assert_same(results[0], results[1])
