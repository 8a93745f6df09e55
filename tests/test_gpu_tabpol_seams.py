"""The seams of the tabular policy kernel (csrc/tabular_policy.hip) that tests/test_gpu_tabpol.py does
not cross: TEST sessions that select with a Softmax, an ExclusiveEpsilonGreedy or a RandomDiscrete
``policy_test`` (``learn == false``, the stream of ``policy_test``), the model digest the kernel
writes where the wavefront kernels consume it (sessions of both kinds interleaved on one agent at
32 x 32), three / five / seven actions, several instances on one parameter set, three worlds with an
instance base that is no multiple of three.  Against the records taken from the reference
(tests/golden/tabpol_sweep_traces.npz) and the restatement of tests/tabpol_common.py."""
import json
import os

import numpy as np
import pytest

import tabpol_common as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'tabpol_sweep_traces.npz'))


@pytest.fixture(scope='module')
def grid4_tables():
    from cobel_amd.misc import gridworld_tools
    return tc.world_tables(tc.grid4(gridworld_tools))


def rebuilt_index(torch, ag):
    from cobel_amd import _lib
    fresh = torch.empty_like(ag.M.index)
    _lib.check(_lib.lib().cobel_model_index_build(_lib.ptr(ag.M.table), _lib.ptr(fresh), ag.n_envs,
                                                  ag.n_states, None))
    torch.cuda.synchronize()
    return fresh


def at_rest(ag, agent) -> dict:
    """What a test session may not touch."""
    from cobel_amd import _lib
    d = dict(Q=ag._q.clone(), policy_counter=ag.policy.counter.clone(), batches_done=ag.batches_done.clone(),
             ctr_memory=ag.inst[:, _lib.I_CTR_MEMORY].clone(), log_len=ag.inst[:, _lib.I_LOG_LEN].clone())
    if agent == 'dynaq':
        d.update(model=ag.M.table.clone(), index=ag.M.index.clone(), M_counter=ag.M.counter.clone())
    else:
        d['log'] = ag._log.clone()
    return d


def assert_at_rest(torch, ag, agent, before, shared: bool):
    after = at_rest(ag, agent)
    for k, was in before.items():
        if k == 'policy_counter' and shared:
            continue                     # (the shared object: its stream goes on)
        assert torch.equal(was, after[k]), 'the test session changed %s' % k


# -- (a) test sessions on the policy kernel -------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(tc.TEST_CASES))
def test_test_session_step_by_step(torch_cuda, Z, name):
    """One instance with step callbacks (a launch per step): the steps of the test session are the
    reference's, and nothing but the environment and the test policy's counter has moved."""
    from cobel_amd import _lib
    c = tc.session_case(name)
    env = tc.device_env('grid4', 1, base=c['inst'])
    ag = tc.device_agent(env, c['agent'], c['policy'], c['test'])
    rec = dict(sarsn=[], steps=[], trial_reward=[])
    ag.callbacks.custom_callbacks = {
        'on_step_end': [lambda logs: rec['sarsn'].append((logs['state'], logs['action'], logs['reward'],
                                                          logs['next_state'], logs['terminal']))],
        'on_trial_end': [lambda logs: (rec['steps'].append(logs['steps']),
                                       rec['trial_reward'].append(logs['trial_reward']))],
        'on_trial_begin': [], 'on_step_begin': []}
    ag.train(env, tc.TRIALS, tc.STEPS, tc.TEST_BATCH)
    n_train = len(rec['sarsn'])
    assert n_train == int(Z[name + '/n_train_steps'])
    plan = ag.describe_launch(env, ag.policy_test, 0, ag.current_trial + 1, tc.TEST_STEPS, 1, 0)
    assert plan['kernel'] == 'policy'
    before = at_rest(ag, c['agent'])
    ag.test(env, tc.TEST_TRIALS, tc.TEST_STEPS)
    assert_at_rest(torch_cuda, ag, c['agent'], before, shared=c['test'] is None)
    a = np.array(rec['sarsn'], dtype=np.float64).reshape(-1, 5)
    assert len(a) > n_train
    for col, k in enumerate(('state', 'action', 'reward', 'next_state', 'nonterminal')):
        assert np.array_equal(a[:, col], Z['%s/%s' % (name, k)].astype(np.float64)), (name, k)
    assert np.array_equal(np.array(rec['steps']), Z[name + '/steps']), name
    assert np.array_equal(np.array(rec['trial_reward'], dtype=np.float64), Z[name + '/trial_reward']), name
    got = tc.device_tables(ag, 0, 4)
    for k in ('Q', 'M_rewards', 'M_states', 'M_terminals', 'log', 'ctr_env', 'ctr_memory'):
        if name + '/' + k in Z.files:
            assert np.array_equal(got[k], Z[name + '/' + k]), (name, k)
    assert int(ag.inst[0, _lib.I_STATE].item()) == int(Z[name + '/env_state'])
    assert int(ag.policy.counter[0].item()) == int(Z[name + '/ctr_policy']), name
    assert ag.policy.stream == _lib.STREAM_POLICY
    if c['test'] is None:      # the shared object continues the training policy's stream
        assert ag.policy_test is ag.policy
        assert int(ag.policy.counter[0].item()) == len(a)
    else:
        assert ag.policy_test.stream == _lib.STREAM_POLICY_TEST
        assert int(ag.policy_test.counter[0].item()) == int(Z[name + '/ctr_policy_test']) == len(a) - n_train


@pytest.mark.parametrize('name', sorted(tc.TEST_CASES))
def test_test_session_in_one_launch(torch_cuda, Z, grid4_tables, name):
    """The same two sessions as ONE launch each among three instances (the case's is the middle
    one): every instance equals the restatement, the middle one the reference's record."""
    from cobel_amd import _lib
    c = tc.session_case(name)
    base = c['inst'] - 1
    env = tc.device_env('grid4', 3, base=base)
    ag = tc.device_agent(env, c['agent'], c['policy'], c['test'])
    ag.train(env, tc.TRIALS, tc.STEPS, tc.TEST_BATCH)
    before = at_rest(ag, c['agent'])
    steps_before = ag.env_steps()
    ag.test(env, tc.TEST_TRIALS, tc.TEST_STEPS)
    assert_at_rest(torch_cuda, ag, c['agent'], before, shared=c['test'] is None)
    refs = [tc.restated_test_case(name, grid4_tables, base + i) for i in range(3)]
    for i, r in enumerate(refs):
        tc.assert_instance(ag, i, r, tc.TEST_BATCH, name)
        want = r.record()
        assert int(ag.inst[i, _lib.I_STATE].item()) == int(want['env_state'])
        if c['test'] is not None:
            assert int(ag.policy_test.counter[i].item()) == int(want['ctr_policy_test'])
    got = tc.device_tables(ag, 1, 4)
    total = tc.TRIALS + tc.TEST_TRIALS
    assert np.array_equal(got['Q'], Z[name + '/Q']) and np.array_equal(got['steps'][:total], Z[name + '/steps'])
    steps = np.array([r.trace['steps'] for r in refs])
    assert np.array_equal(ag.monitors.lat_sum.cpu().numpy()[:total], steps.sum(axis=0))
    assert np.array_equal(ag.monitors.lat_cnt.cpu().numpy()[:total], np.full(total, 3))
    rew = np.array([r.trace['trial_reward'] for r in refs])      # (rewards 0 and 1: exact in any order)
    assert np.array_equal(ag.monitors.reward_sum.cpu().numpy()[:total], rew.sum(axis=0))
    assert ag.env_steps() - steps_before == int((steps[:, tc.TRIALS:] + 1).sum())
    if c['test'] is not None:
        assert ag.policy_test.stream == _lib.STREAM_POLICY_TEST and ag.policy.stream == _lib.STREAM_POLICY


# -- (b) sessions of both kinds interleaved where the digest is consumed ----------------------------------------------
CROSSING = {'dynaq_softmax': ('dynaq', (tc.SOFTMAX, 2.0)), 'q_exclusive': ('q', (tc.EXCLUSIVE, 0.3))}


@pytest.mark.parametrize('name', sorted(CROSSING))
def test_sessions_interleave_at_32x32(torch_cuda, name):
    """Three instances (instance_base 5) on the 32 x 32 open field, batch 8, three sessions of
    2 trials x 40 steps on ONE agent: EpsilonGreedy(0.1), the policy kernel, the same EpsilonGreedy
    again (``agent.policy`` assigned for each).  Dyna-Q's EpsilonGreedy sessions take the
    persistent-workgroup kernel, which reads the digest — after the second session the one the
    policy kernel wrote.  After each session every instance equals the restatement and ``M.index``
    is the digest of ``M.table``."""
    from cobel_amd import _lib
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc import gridworld_tools
    from oracle.philox import STREAM_POLICY
    agent, middle = CROSSING[name]
    n, base, batch, trials, steps = 3, 5, 8, 2, 40
    # (the open field of make_open_field(32, 32, 0, 1) with starts near its goal, so that the short
    #  sessions meet the reward and the digest's reward bit is set by both kinds of kernel)
    world = gridworld_tools.make_gridworld(32, 32, terminals=[0], rewards=np.array([[0, 1.0]]), goals=[0],
                                           starting_states=[1, 2, 32, 33, 34, 65])
    env = Gridworld(world, n_envs=n, seed=tc.SEED, instance_base=base)
    ag = tc.device_agent(env, agent, ('eps', 0.1))
    eps, other = ag.policy, tc.device_policy(middle, 4)
    tabs = tc.world_tables(world)
    refs = [tc.Restated(tabs, agent, ('eps', 0.1), base + i) for i in range(n)]
    ref_other = [r.policy_object(middle, STREAM_POLICY) for r in refs]
    with open(os.path.join(GOLDEN, 'tab_routing.json')) as f:
        table = json.load(f)
    witness = {r['name']: r['out'] for r in table['rows']}['s1024_a4_w1/dyna_b32_midx']
    ag._bind(env)
    for k, pol in enumerate((eps, other, eps)):
        plan = ag.describe_launch(env, pol, _lib.F_LEARN, ag.current_trial + trials, steps, 0, batch)
        if pol is other:
            assert plan['kernel'] == 'policy'
        elif agent == 'dynaq':
            assert plan['kernel'] == witness[0] == _lib.TAB_KERNEL_PWG, 'the kernel that reads the digest'
        else:
            assert plan['kernel'] != 'policy'
        ag.policy = pol
        ag.train(env, trials, steps, batch)
        for i, r in enumerate(refs):
            r.session(r.pol if pol is eps else ref_other[i], trials, steps, batch, True)
            want, got = r.record(), tc.device_tables(ag, i, 4)
            for key in ('Q', 'M_rewards', 'M_states', 'M_terminals', 'log', 'ctr_env', 'ctr_memory'):
                if key in want:
                    assert np.array_equal(got[key], want[key]), (name, k, i, key)
            done = (k + 1) * trials
            assert np.array_equal(got['steps'][:done], want['steps']), (name, k, i)
            assert int(eps.counter[i].item()) == r.pol.rng.index, (name, k, i)
            assert int(0 if other.counter is None else other.counter[i].item()) == ref_other[i].rng.index
        if agent == 'dynaq':
            assert torch_cuda.equal(rebuilt_index(torch_cuda, ag), ag.M.index), (name, k)
    assert eps.stream == other.stream == _lib.STREAM_POLICY
    assert all(np.any(r.ag.Q != 0) for r in refs), 'every instance met the reward'


# -- (b2) a draw that lies ON an edge of its CDF ---------------------------------------------------------------------
def test_a_draw_on_an_edge_takes_the_action_to_its_right(torch_cuda):
    """Generator.choice is ``searchsorted(cdf, u, side='right')``: a draw equal to an edge belongs to
    the action to the right of it.  The streams never hand out such a draw, so the rows are planted
    (``cobel_policy_select_n``, the selection the run kernel shares): edges that are exact in binary,
    among them the edge 0 behind actions of probability zero, which ``u = 0`` may not select."""
    from cobel_amd import _lib
    from cobel_amd.policy.greedy import select_n
    dev = torch_cuda.device('cuda', 0)
    rows = [  # values, epsilon, draw, the action
        ([0.0, 1.0, 0.0, 0.0], 0.0, 0.0, 1),      # cdf 0 1 1 1
        ([0.0, 0.0, 0.0, 1.0], 0.0, 0.0, 3),      # cdf 0 0 0 1
        ([1.0, 0.0, 0.0, 0.0], 0.75, 0.25, 1),    # cdf .25 .5 .75 1
        ([1.0, 0.0, 0.0, 0.0], 0.75, 0.5, 2),
        ([1.0, 0.0, 0.0, 0.0], 0.75, 0.75, 3),
        ([1.0, 1.0, 0.0, 0.0], 0.5, 0.5, 2),      # cdf .25 .5 .75 1, two ties
    ]
    v = torch_cuda.tensor([r[0] for r in rows], dtype=torch_cuda.float64, device=dev)
    eps = torch_cuda.tensor([r[1] for r in rows], dtype=torch_cuda.float64, device=dev)
    u = torch_cuda.tensor([r[2] for r in rows], dtype=torch_cuda.float64, device=dev)
    act, probs = select_n(_lib.POLICY_EXCLUSIVE, v, None, u, None, eps, len(rows), 4, dev)
    act, probs = act.cpu().numpy(), probs.cpu().numpy()
    for j, (values, e, draw, want) in enumerate(rows):
        p = tc.exclusive_probs(np.array(values), e)
        cdf = tc.cdf_of(p)
        assert draw in cdf and np.array_equal(probs[j], p), j
        assert want == int(np.searchsorted(cdf, draw, side='right')) == act[j], (j, act[j])
        assert p[act[j]] > 0.0
    # Softmax: two equal values, the edge 0.5 exactly
    v2 = torch_cuda.tensor([[0.3, 0.3]], dtype=torch_cuda.float64, device=dev)
    u2 = torch_cuda.tensor([0.5], dtype=torch_cuda.float64, device=dev)
    beta = torch_cuda.tensor([2.0], dtype=torch_cuda.float64, device=dev)
    act, probs = select_n(_lib.POLICY_SOFTMAX, v2, None, u2, None, beta, 1, 2, dev)
    assert np.array_equal(probs.cpu().numpy()[0], [0.5, 0.5]) and int(act.cpu().numpy()[0]) == 1


# -- (c) odd action counts, shared parameter sets, three worlds -------------------------------------------------------
@pytest.fixture(scope='module')
def sweeps():
    """The restatement of every sweep, computed once and left unchanged."""
    from cobel_amd.misc import gridworld_tools
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tc.restate_sweep(name, gridworld_tools)
        return cache[name]
    return get


def device_sweep(name):
    from cobel_amd.interface import Gridworld, Topology
    from cobel_amd.misc import gridworld_tools
    s = tc.sweep(name)
    descr = [tc.sweep_world(w, gridworld_tools)[0] for w in s['worlds']]
    if descr[0][0] == 'nodes':
        env = Topology(descr[0][1], descr[0][2], n_envs=s['n'], seed=tc.SEED, instance_base=s['base'])
    else:
        worlds = [d[1] for d in descr]
        env = Gridworld(worlds if len(worlds) > 1 else worlds[0], n_envs=s['n'], seed=tc.SEED,
                        instance_base=s['base'])
    p = tc.sweep_params(s)
    ag = tc.device_agent(env, s['agent'], (s['kind'], p['par']), alpha=p['alpha'], gamma=p['gamma'])
    return s, env, ag


@pytest.mark.parametrize('name', sorted(tc.SEAM_SWEEPS))
def test_odd_widths_shared_sets_and_three_worlds(torch_cuda, sweeps, name):
    from cobel_amd import _lib
    s, env, ag = device_sweep(name)
    ag._bind(env)
    plan = ag.describe_launch(env, ag.policy, _lib.F_LEARN, s['trials'], s['steps'], 0, s['batch'])
    assert plan['kernel'] == 'policy'
    if name.startswith('a'):
        assert int(env.action_space.n) == int(name[1]) and int(name[1]) in (3, 5, 7)
    if name.startswith('shared'):
        assert ag._ppol[3] == 3, 'nine instances on three parameter sets'
        assert np.array_equal(np.unique(ag._ppol[2].cpu().numpy(), return_counts=True)[1], [3, 3, 3])
    if name.startswith('three_worlds'):
        assert env.handle.n_worlds == 3 and s['base'] % 3 != 0
    ag.train(env, s['trials'], s['steps'], s['batch'])
    refs = sweeps(name)
    assert len(refs) == s['n']
    for i, r in refs.items():
        tc.assert_instance(ag, i, r, s['batch'], name)
    if s['kind'] != tc.RANDOM:
        assert any(np.any(r.ag.Q != 0) for r in refs.values()), 'somebody learnt something'
    if s['agent'] == 'dynaq':
        assert torch_cuda.equal(rebuilt_index(torch_cuda, ag), ag.M.index)
