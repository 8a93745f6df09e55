"""GPU tests of the MFEC agent: the device against the traces recorded from the real reference
(tests/golden/mfec_traces.npz) and against the NumPy restatement (tests/mfec_common.py) on shapes
the fixture does not hold.  Every comparison is bit-exact (np.array_equal); no case is left out of
the strict comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfec_common as mc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xC0BE1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mfec_traces.npz')
CASES = ['track_k3_c12', 'grid5_k10_c80', 'hex4_k2_c10', 'grid5_timeouts', 'track_c2_k3',
         'track_dict', 'track_traintest']


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


def graph(name):
    from cobel_amd.misc import topology_tools as tt
    if name == 'track':
        return tt.linear_track(10, 2, 1.0, 20, 'right')
    if name.startswith('grid'):
        return tt.grid(int(name[4:]), (0.0, 1.0))
    return tt.hexagonal(int(name[3:]), (0.0, 1.0))


def make_env(gname, okind='onehot', n=1, base=0, nodes=None, starts=None):
    from cobel_amd.interface import Topology
    from cobel_amd.interface.simulator.offline import OfflineSimulator
    from cobel_amd.spaces import Box, Dict
    if nodes is None:
        nodes, starts = graph(gname)
    ids = list(nodes)
    S = len(ids)
    if okind == 'dict':
        obs = {tuple(nodes[k]['pose']): {'1': np.array(nodes[k]['pose']), '2': np.array(nodes[k]['pose'])}
               for k in ids}
        space = Dict({'1': Box(0., 1., (6,)), '2': Box(0., 1., (6,))})
    else:
        obs = {tuple(nodes[k]['pose']): o for k, o in zip(ids, np.eye(S))}
        space = Box(low=0.0, high=1.0, shape=(S,))
    return Topology(nodes, starts, OfflineSimulator(obs, space), n_envs=n, seed=SEED,
                    instance_base=base)


def tab_of(env):
    w = env._tables()
    return {'next': w['next'], 'reward': np.asarray(w['rewards'], dtype=np.float64),
            'terminal': np.asarray(w['terminals']).astype(np.uint8),
            'starts': np.asarray(w['starting_states']).astype(np.uint16)}


def make_agent(env, capacity, k, eps, inst, features=None, record=20000):
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    ag = MFEC(env.observation_space, env.action_space, EpsilonGreedy(eps), capacity=capacity, k=k,
              projection_size=16, rng=np.random.default_rng(inst))
    ag.record_steps = record
    if features is not None:
        ag.feature_table = lambda interface: np.ascontiguousarray(features)
    return ag


class Recorder:
    """The record of mfec_common.pack from a single-instance device agent."""

    def __init__(self, agent):
        self.agent, self.tr = agent, mc.new_trace()
        agent.callbacks.custom_callbacks = {'on_trial_end': [self.on_trial_end]}

    def on_trial_end(self, logs):
        self.tr['steps'].append(int(logs['steps']))
        mc.snapshot(self.tr, logs['agent'].Q.buffers)

    def pack(self, env):
        ag, tr = self.agent, self.tr
        A = ag.n_actions
        rows = ag.recorded_steps(0)
        tr['sar'] = [tuple(r[:4]) for r in rows]
        tr['q'] = [r[4:] for r in rows]
        at = 0
        for lat in tr['steps']:
            at += lat + 1
            tr['ended'].append(bool(rows[at - 1][3]))
        assert at == len(rows)
        out = mc.pack(tr, A)
        out['index'] = np.array([int(env.env_ctr[0].item()), int(ag.policy.counter[0].item())],
                                dtype=np.int64)
        out['predict'] = ag.predict_on_batch(list(range(ag.n_states)))
        return out


def device_case(env, cfg, features=None, gamma=None):
    inst, trials, steps, capacity, k, test_trials, eps6 = [int(x) for x in cfg]
    ag = make_agent(env, capacity, k, eps6 / 1e6, inst, features)
    if gamma is not None:
        ag.gamma = gamma
    rec = Recorder(ag)
    ag.train(env, trials, steps)
    if test_trials:
        ag.test(env, test_trials, steps)
    return rec.pack(env), ag


# -- against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_device_reproduces_the_reference(Z, name):
    """Steps, estimates, buffers after every trial, generator indices and predict_on_batch of every
    recorded case.  The feature table is the recorded one (np.dot's summation order may differ
    between BLAS builds in the last bit; the agent's own table is checked to agree to 1e-12 and, on
    one machine, bit for bit in test_host_mfec.py)."""
    cfg = Z[name + '/cfg']
    env = make_env(str(Z[name + '/graph']), str(Z[name + '/observations']), base=int(cfg[0]))
    tab = tab_of(env)
    for k in tab:
        assert np.array_equal(tab[k], Z['%s/tab_%s' % (name, k)]), k
    from cobel_amd.agent import MFEC
    from cobel_amd.policy import EpsilonGreedy
    probe = MFEC(env.observation_space, env.action_space, EpsilonGreedy(0.1), projection_size=16,
                 rng=np.random.default_rng(int(cfg[0])))
    assert np.array_equal(probe.projection, Z[name + '/projection'])
    assert np.allclose(probe.feature_table(env), Z[name + '/F'], rtol=1e-12, atol=0)
    out, ag = device_case(env, cfg, features=Z[name + '/F'], gamma=float(Z[name + '/gamma']))
    mc.assert_same_record(out, Z, name + '/', what=name)


# -- against the restatement ----------------------------------------------------------------------
def both(gname, cfg, okind='onehot'):
    env = make_env(gname, okind, base=int(cfg[0]))
    out, ag = device_case(env, cfg)
    ref, rag = mc.run_restatement(tab_of(env), ag.features, cfg, SEED)
    return out, ref, ag


SHAPES = {
    # name: (graph, [instance, trials, steps, capacity, k, test trials, epsilon x 1e6])
    'capacity3_k2': ('track', [11, 25, 120, 3, 2, 0, 100000]),
    'capacity1': ('track', [12, 25, 120, 1, 1, 0, 100000]),
    'grid9_capacity67': ('grid9', [13, 70, 60, 67, 3, 0, 300000]),       # crosses one wavefront
    'grid9_capacity130': ('grid9', [14, 220, 60, 130, 5, 0, 500000]),    # above 80: the restatement rules
    'hex5_six_actions': ('hex5', [15, 40, 40, 20, 4, 0, 100000]),
    'all_time_out': ('track', [16, 12, 3, 12, 3, 0, 100000]),
    'k32': ('grid9', [17, 70, 60, 70, 32, 0, 300000]),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_device_equals_restatement(name):
    gname, cfg = SHAPES[name]
    out, ref, ag = both(gname, cfg)
    mc.assert_same_record(out, ref, what=name)
    lens = out['buf_len']
    if name == 'grid9_capacity67':
        assert lens.max() >= 65, lens.max()
    if name == 'grid9_capacity130':
        assert lens.max() > 80, lens.max()
    if name == 'hex5_six_actions':
        assert ag.n_actions == 6 and out['ended'].any()
    if name == 'all_time_out':
        assert not out['ended'].any() and not lens.any() and not out['q'].any()
    if name == 'capacity1':
        assert lens.max() == 1
    if name == 'k32':
        assert lens.max() > 32 and (out['q'] != 0).any()
    assert ag.n_states < 64 or gname == 'grid9'      # (track, hex5: fewer nodes than lanes)


@pytest.mark.parametrize('n', [1, 2, 65])
def test_instances_of_one_launch_equal_their_own_runs(n):
    """Distinct streams per instance; every instance looked at equals the single-instance run with
    its instance number."""
    cfg = [0, 20, 120, 12, 3, 0, 100000]
    env = make_env('track', n=n, base=3)
    ag = make_agent(env, 12, 3, 0.1, 3, record=0)
    ag.track_instances = True
    ag.train(env, 20, 120)
    lat = ag.monitors.lat_trace.cpu().numpy()
    seen = set()
    for i in sorted({0, n - 1, n // 2}):
        one = make_env('track', base=3 + i)
        solo = make_agent(one, 12, 3, 0.1, 3, record=0)
        solo.track_instances = True
        solo.train(one, 20, 120)
        assert np.array_equal(solo.monitors.lat_trace.cpu().numpy()[0], lat[i])
        for a, b in zip(solo.memory(0).buffers, ag.memory(i).buffers):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        assert np.array_equal(solo.predict_on_batch(range(20)),
                              ag.predict_on_batch(range(20))[i].cpu().numpy() if n > 1
                              else ag.predict_on_batch(range(20)))
        seen.add(lat[i].tobytes())
    assert len(seen) == len({0, n - 1, n // 2}), 'the instances ran the same stream'
    assert cfg[3] == 12


def test_two_train_calls_equal_one_of_the_summed_length():
    runs = []
    for parts in ((30,), (12, 18)):
        env = make_env('track', base=21)
        ag = make_agent(env, 12, 3, 0.1, 21)
        for t in parts:
            ag.train(env, t, 100)
        runs.append((ag.recorded_steps(0), [tuple(b) for b in ag.Q.buffers], ag.current_trial))
    assert runs[0][2] == runs[1][2] == 30
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_test_leaves_the_buffers_untouched():
    env = make_env('track', base=22)
    ag = make_agent(env, 12, 3, 0.1, 22)
    ag.train(env, 20, 120)
    before = [tuple(b) for b in ag.Q.buffers]
    clock = int(ag._clock[0].item())
    assert sum(len(b[0]) for b in before) > 0
    ag.test(env, 10, 120)
    assert ag.current_trial == 30 and int(ag._clock[0].item()) == clock
    for a, b in zip(before, [tuple(b) for b in ag.Q.buffers]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_live_world_edit_between_two_sessions():
    """The goal moves between two train() calls (a node's reward and terminal flag are edited, as a
    user edits a Topology): the device follows as the restatement does on the edited tables."""
    from oracle.philox import STREAM_ENV, STREAM_POLICY, TapeRNG
    from oracle.ref_loop import RefEpsilonGreedy, RefGridworld
    inst = 23
    env = make_env('grid5', base=inst)
    ag = make_agent(env, 30, 3, 0.2, inst)
    rec = Recorder(ag)
    ag.train(env, 25, 40)
    tab0 = tab_of(env)
    goal = int(np.flatnonzero(tab0['terminal'])[0])
    new = 12 if goal != 12 else 0
    ids = env.ids
    env.nodes[ids[goal]]['reward'], env.nodes[ids[goal]]['terminal'] = 0.0, False
    env.nodes[ids[new]]['reward'], env.nodes[ids[new]]['terminal'] = 1.0, True
    ag.train(env, 25, 40)
    out = rec.pack(env)
    tab1 = tab_of(env)
    assert int(np.flatnonzero(tab1['terminal'])[0]) == new
    renv = RefGridworld(tab0, TapeRNG(SEED, inst, STREAM_ENV))
    pol = RefEpsilonGreedy(0.2, TapeRNG(SEED, inst, STREAM_POLICY))
    rag = mc.RefMFEC(ag.features, ag.n_actions, pol, capacity=30, k=3)
    tr = mc.new_trace()
    rag.train(renv, 25, 40, trace=tr)
    renv.reward, renv.terminal = tab1['reward'], tab1['terminal']
    rag.train(renv, 25, 40, trace=tr)
    ref = mc.pack(tr, ag.n_actions)
    ref['index'] = np.array([renv.rng.index, pol.rng.index], dtype=np.int64)
    ref['predict'] = rag.predict_on_batch(range(ag.n_states))
    mc.assert_same_record(out, ref, what='live edit')
    assert out['ended'][25:].any()


def test_callbacks_per_step_equal_the_fused_run():
    """Step callbacks make the agent launch once per step (as the other fused agents do): the same
    steps, the same memory."""
    runs = []
    for per_step in (False, True):
        env = make_env('track', base=24)
        ag = make_agent(env, 12, 3, 0.1, 24)
        seen = []
        if per_step:
            ag.callbacks.custom_callbacks = {'on_step_end': [lambda logs: seen.append(
                (logs['state'], logs['action'], logs['reward'], 1 - logs['terminal']))]}
        ag.train(env, 6, 60)
        rows = ag.recorded_steps(0)
        if per_step:
            assert np.array_equal(np.array(seen, dtype=np.float64), rows[:, :4])
        runs.append((rows, [tuple(b) for b in ag.Q.buffers]))
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# -- the pair tables --------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 16, 256])
def test_pair_tables_equal_the_sequential_sum(D):
    import torch
    from cobel_amd import _lib
    S = 37
    rng = np.random.default_rng(D)
    F = rng.random((S, D))
    F[5] = F[4]                              # a duplicate row: distance exactly 0, allclose both ways
    F[7] = F[6] * (1 + 9e-5) + 5e-7          # allclose, not equal
    F[9] = F[8] * (1 + 2e-4)                 # outside the tolerance
    dev = torch.device('cuda', torch.cuda.current_device())
    f = torch.as_tensor(F, device=dev)
    r = torch.zeros((S, S), dtype=torch.float64, device=dev)
    s = torch.zeros((S, S), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().cobel_mfec_pairs(_lib.ptr(f), S, D, _lib.ptr(r), _lib.ptr(s),
                                           _lib.current_stream(dev)))
    R, same = mc.pair_tables(F)
    assert np.array_equal(r.cpu().numpy(), R)
    assert np.array_equal(s.cpu().numpy().astype(bool), same)
    assert same[4, 5] and same[6, 7] and not same[8, 9] and R[4, 5] == 0.0


def test_nodes_that_are_allclose_are_refused():
    env = make_env('track', base=25)
    F = np.random.default_rng(0).random((20, 16))
    F[3] = F[2] * (1 + 5e-5)
    ag = make_agent(env, 12, 3, 0.1, 25, features=F)
    with pytest.raises(NotImplementedError, match='allclose'):
        ag.train(env, 1, 10)
