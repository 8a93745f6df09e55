"""QAgent and DynaQ with a Softmax, an ExclusiveEpsilonGreedy or a RandomDiscrete policy on the
device (csrc/tabular_policy.hip, cobel_tab_policy_run / cobel_policy_select_n): against traces
recorded from the reference, against the NumPy restatement at the kernel's seams, on planted rows,
inside sentinel frames, and beside the epsilon-greedy path, which must not have moved."""
import ctypes as C
import os

import numpy as np
import pytest

import frames_common as fc
import tabpol_common as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# Softmax probabilities of the device against NumPy's, relative.  Measured on this module's
# known-answer set (the rows of the fixture and the planted rows below): 3.08e-16 = 2**-51.53
# (docs/MEASUREMENTS.md section 32); the bound is the next power of two above the measured figure
# and has to stay below 2**-48, the project's criterion (section 24).
SOFTMAX_REL_BOUND = 2.0 ** -51


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


@pytest.fixture(scope='module')
def Z():
    return np.load(os.path.join(GOLDEN, 'tabpol_traces.npz'))


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


# -- (a) the traces ---------------------------------------------------------------------------------------------
def run_case_per_step(name):
    """The case on one device instance with step and trial callbacks: a launch per step."""
    c = tc.case(name)
    opt = c['opt']
    env = tc.device_env(c['world'], 1, base=c['inst'])
    mask = tc.two_action_mask(np.zeros((16, 4))) if opt.get('mask') else None
    ag = tc.device_agent(env, c['agent'], c['policy'], opt.get('test'), mask=mask)
    rec = dict(sarsn=[], td=[], steps=[], trial_reward=[], Q_trial=[])
    ag.callbacks.custom_callbacks = {
        'on_step_end': [lambda logs: (rec['sarsn'].append((logs['state'], logs['action'], logs['reward'],
                                                           logs['next_state'], logs['terminal'])),
                                      rec['td'].append(logs.get('td', 0.0)))],
        'on_trial_end': [lambda logs: (rec['steps'].append(logs['steps']),
                                       rec['trial_reward'].append(logs['trial_reward']),
                                       rec['Q_trial'].append(np.array(ag.Q, dtype=np.float32)))],
        'on_trial_begin': [], 'on_step_begin': []}
    if c['agent'] == 'dynaq':
        ag.train(env, tc.TRIALS, tc.STEPS, c['batch'], bool(opt.get('no_replay')))
    else:
        ag.train(env, tc.TRIALS, tc.STEPS, c['batch'])
    if opt.get('test'):
        ag.test(env, tc.TRIALS, tc.STEPS)
    return ag, rec


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_traces_step_by_step(torch_cuda, Z, name):
    """Per step, per trial and per session: states, actions, rewards, td (Dyna-Q), Q after every
    trial, the model / the log, the counters.  The last case crosses from the new kernel (training
    with Softmax) to an existing one (testing with EpsilonGreedy) on the same tables."""
    from cobel_amd import _lib
    c = tc.case(name)
    ag, rec = run_case_per_step(name)
    want = {k: Z['%s/%s' % (name, k)] for k in tc.EXACT if '%s/%s' % (name, k) in Z.files}
    a = np.array(rec['sarsn'], dtype=np.float64).reshape(-1, 5)
    for col, k in enumerate(('state', 'action', 'reward', 'next_state', 'nonterminal')):
        assert np.array_equal(a[:, col], want[k].astype(np.float64)), (name, k)
    if c['agent'] == 'dynaq':
        assert np.array_equal(np.array(rec['td'], dtype=np.float64), want['td']), name
    assert np.array_equal(np.array(rec['steps']), want['steps']), name
    assert np.array_equal(np.array(rec['trial_reward'], dtype=np.float64), want['trial_reward']), name
    assert np.array_equal(np.array(rec['Q_trial'], dtype=np.float32), want['Q_trial']), name
    got = tc.device_tables(ag, 0, want['Q'].shape[1])
    for k in ('Q', 'M_rewards', 'M_states', 'M_terminals', 'log', 'ctr_env', 'ctr_memory'):
        if k in want and not (k == 'ctr_memory' and c['batch'] == 0):
            assert np.array_equal(got[k], want[k]), (name, k)
    assert int(ag.policy.counter[0].item()) == int(want['ctr_policy']), name
    if c['opt'].get('test'):
        assert ag.policy_test.stream == _lib.STREAM_POLICY_TEST
        assert int(ag.policy_test.counter[0].item()) == int(want['ctr_policy_test']), name


@pytest.mark.parametrize('name', sorted(tc.CASES))
def test_traces_in_one_launch_and_monitors(torch_cuda, Z, name):
    """The same sessions as ONE launch each among three instances (the case's is the middle one),
    with the sums of RewardMonitor / EscapeLatencyMonitor over the instances."""
    from cobel_amd.misc import gridworld_tools, topology_tools
    c = tc.case(name)
    opt = c['opt']
    base = c['inst'] - 1 if c['inst'] else 0
    mid = c['inst'] - base
    env = tc.device_env(c['world'], 3, base=base)
    tabs = tc.case_tables(c, gridworld_tools, topology_tools)
    mask = tc.two_action_mask(tabs['next']) if opt.get('mask') else None
    ag = tc.device_agent(env, c['agent'], c['policy'], opt.get('test'), mask=mask)
    refs = [tc.Restated(tabs, c['agent'], c['policy'], base + i, test_policy=opt.get('test'), mask=mask)
            for i in range(3)]
    if c['agent'] == 'dynaq':
        ag.train(env, tc.TRIALS, tc.STEPS, c['batch'], bool(opt.get('no_replay')))
    else:
        ag.train(env, tc.TRIALS, tc.STEPS, c['batch'])
    for r in refs:
        r.train(tc.TRIALS, tc.STEPS, c['batch'], bool(opt.get('no_replay')))
    if opt.get('test'):
        ag.test(env, tc.TRIALS, tc.STEPS)
        for r in refs:
            r.test(tc.TRIALS, tc.STEPS)
    for i, r in enumerate(refs):
        tc.assert_instance(ag, i, r, c['batch'], name)
    got = tc.device_tables(ag, mid, tabs['next'].shape[1])
    assert np.array_equal(got['Q'], Z[name + '/Q']) and np.array_equal(got['steps'], Z[name + '/steps'])
    steps = np.array([r.trace['steps'] for r in refs])
    rew = np.array([r.trace['trial_reward'] for r in refs])
    assert np.array_equal(ag.monitors.lat_sum.cpu().numpy()[:steps.shape[1]], steps.sum(axis=0))
    assert np.array_equal(ag.monitors.lat_cnt.cpu().numpy()[:steps.shape[1]], np.full(steps.shape[1], 3))
    # (the rewards of these worlds are 0 and 1: their float64 sums are exact in any order)
    assert np.array_equal(ag.monitors.reward_sum.cpu().numpy()[:steps.shape[1]], rew.sum(axis=0))
    assert ag.env_steps() == int((steps + 1).sum())


# -- (b) the seams ----------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize('name', sorted(tc.SWEEPS))
def test_seams_equal_the_restatement(torch_cuda, sweeps, name):
    """130 parameter sets, a tail instance behind full workgroups, two worlds without a shared copy,
    instance_base != 0, one / two / eight actions, one state, 1 024 states, batch 0 / 1 / 62."""
    from cobel_amd import _lib
    s, env, ag = device_sweep(name)
    flags = _lib.F_LEARN
    ag._bind(env)
    plan = ag.describe_launch(env, ag.policy, flags, s['trials'], s['steps'], 0, s['batch'])
    assert plan['kernel'] == 'policy' and plan['threads_per_workgroup'] == 64 * plan['instances_per_workgroup']
    assert plan['workgroups'] == -(-s['n'] // plan['instances_per_workgroup'])
    if name.startswith('tail'):
        assert plan['instances_per_workgroup'] > 1 and (s['n'] - 1) % plan['instances_per_workgroup'] == 0
    if name.startswith('two_worlds'):
        assert env.handle.n_worlds == 2
    if name.startswith('sets'):
        ag.describe_launch(env, ag.policy, flags, s['trials'], s['steps'], 0, s['batch'])
        assert ag._ppol[3] == s['n'], 'every instance is a parameter set of its own'
    if s['agent'] == 'dynaq':
        ag.train(env, s['trials'], s['steps'], s['batch'])
    else:
        ag.train(env, s['trials'], s['steps'], s['batch'])
    for i, r in sweeps(name).items():
        tc.assert_instance(ag, i, r, s['batch'], name)
    if name.startswith('s1024'):
        assert ag.n_states == 1024
    if s['batch'] == 0 and s['agent'] == 'dynaq':
        assert int(ag.batches_done.item()) == 0


# -- (c) planted rows -------------------------------------------------------------------------------------------
def select_n(torch, policy, v, bits, u, k, par, A):
    from cobel_amd import _lib
    from cobel_amd.policy.greedy import select_n as call
    dev = torch.device('cuda', 0)
    t = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dt).contiguous()  # noqa: E731
    n = len(u) if u is not None else len(k)
    kk = None if k is None else torch.as_tensor(np.asarray(k, dtype=np.uint64).astype(np.int64), device=dev)
    act, probs = call(policy, t(v, torch.float64), t(bits, torch.uint8), t(u, torch.float64), kk,
                      t(par, torch.float64), n, A, dev)
    return act.cpu().numpy(), probs.cpu().numpy()


def test_planted_rows_exclusive(torch_cuda):
    """Every value tied (the max(..., 1) branch), epsilon 0 and 1, masks that leave one action, the
    two ends of the draw's range: probabilities and actions exact."""
    from cobel_amd import _lib
    rows = [([0.5] * 4, 0xF), ([0.5, 0.5, 0.25, 0.5], 0xF), ([1.0, 2.0, 2.0, -1.0], 0xF),
            ([1.0, 2.0, 3.0, 4.0], 0x4), ([1.0, 2.0, 3.0, 4.0], 0x1), ([0.0, 0.0, 1.0, 1.0], 0x3),
            ([-1.0, -1.0, -1.0, -1.0], 0xA)]
    us = [0.0, np.nextafter(1.0, 0.0), 0.3, 0.5, 0.7]
    for eps in (0.0, 1.0, 0.3):
        v = np.array([r[0] for r in rows for _ in us])
        bits = np.array([r[1] for r in rows for _ in us], dtype=np.uint8)
        u = np.array([x for _ in rows for x in us])
        act, probs = select_n(torch_cuda, _lib.POLICY_EXCLUSIVE, v, bits, u, None, [eps], 4)
        for j in range(len(u)):
            m = np.array([(bits[j] >> a) & 1 for a in range(4)], dtype=bool)
            p = tc.exclusive_probs(v[j].astype(np.float32), eps, m)
            assert probs[j].tobytes() == p.tobytes(), (eps, j)
            if p.sum() == 0.0:      # epsilon 1 and nothing but ties: no action has a probability
                continue            # (Generator.choice raises there; the kernel returns action 0)
            assert act[j] == int(np.searchsorted(tc.cdf_of(p), u[j], side='right')), (eps, j)
            assert m[act[j]] and p[act[j]] > 0.0
    # all tied: the greedy share alone, spread over the ties
    _, probs = select_n(torch_cuda, _lib.POLICY_EXCLUSIVE, [[0.5] * 4], [0xF], [0.1], None, [0.3], 4)
    assert np.array_equal(probs[0], np.full(4, (1.0 - 0.3) / 4))


def test_planted_rows_softmax_and_the_measured_bound(torch_cuda, Z):
    """beta = 1e4 with gaps that underflow (exact zeros, never selected), masks that leave one
    action, u = 0 and u = nextafter(1, 0); on the whole known-answer set the probabilities within
    SOFTMAX_REL_BOUND of NumPy's and the actions the restatement's where the margin allows."""
    from cobel_amd import _lib
    R = {k[5:]: Z[k] for k in Z.files if k.startswith('rows/')}
    sets = []      # (values [n, A], bits, beta)
    for a in range(1, 9):
        sel = np.flatnonzero(R['A'] == a)
        sets.append((R['v'][sel, :a], R['bits'][sel], R['beta'][sel]))
    hot = np.array([[0.7, 0.1, -0.3, 0.6999], [0.7, 0.7, 0.0, -5.0], [0.0, 1.0, 2.0, 3.0]])
    sets.append((hot, np.array([0xF, 0xF, 0xF], dtype=np.uint8), np.full(3, 1e4)))
    one = np.array([[0.1, 2.0, 0.7, 0.3]] * 4)
    sets.append((one, np.array([1, 2, 4, 8], dtype=np.uint8), np.full(4, 5.0)))
    worst = 0.0
    for v, bits, beta in sets:
        n, a = v.shape
        for u0 in (0.0, np.nextafter(1.0, 0.0), 0.37):
            u = np.full(n, u0)
            act, probs = select_n(torch_cuda, _lib.POLICY_SOFTMAX, v, bits, u, None, beta, a)
            for j in range(n):
                m = np.array([(int(bits[j]) >> k) & 1 for k in range(a)], dtype=bool)
                p = tc.softmax_probs(v[j], beta[j], m)
                assert np.array_equal(probs[j] == 0.0, p == 0.0), 'the exact zeros'
                nz = p > 0.0
                worst = max(worst, float(np.max(np.abs(probs[j][nz] - p[nz]) / p[nz])))
                assert m[act[j]] and probs[j][act[j]] > 0.0, 'a masked or impossible action'
                cdf = tc.cdf_of(p)
                if a == 1 or np.abs(cdf[:-1] - u0).min() > 1e-12:
                    assert act[j] == int(np.searchsorted(cdf, u0, side='right'))
                if u0 == 0.0:
                    assert act[j] == int(np.flatnonzero(p > 0.0)[0])
    print('softmax: largest relative difference to NumPy %.3g = 2**%.2f' % (worst, np.log2(worst) if worst else -np.inf))
    assert worst <= SOFTMAX_REL_BOUND < 2.0 ** -48
    # the rows of beta = 1e4: gaps of 0.1 and more underflow to exact zeros
    _, probs = select_n(torch_cuda, _lib.POLICY_SOFTMAX, hot, [0xF] * 3, [0.5] * 3, None, [1e4], 4)
    assert probs[0][1] == 0.0 and probs[0][2] == 0.0 and probs[0][3] > 0.0
    assert np.array_equal(probs[1], [0.5, 0.5, 0.0, 0.0]) and np.array_equal(probs[2], [0.0, 0.0, 0.0, 1.0])


def test_planted_rows_random_and_the_classes(torch_cuda):
    """RandomDiscrete: (word * A) >> 32 exactly, full(A, 1 / A); the policy classes on single rows,
    batches and their own stream."""
    from cobel_amd import _lib
    from cobel_amd.policy import ExclusiveEpsilonGreedy, RandomDiscrete
    from oracle.philox import STREAM_POLICY, draw_bounded, draw_double
    words = np.array([0, 1, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 0x55555555, 0xAAAAAAAB, 123456789], dtype=np.uint64)
    for a in (1, 2, 3, 6, 8):
        act, probs = select_n(torch_cuda, _lib.POLICY_RANDOM, None, None, None, words, None, a)
        assert np.array_equal(act, (words * np.uint64(a)) >> np.uint64(32))
        assert np.array_equal(probs, np.full((len(words), a), 1.0 / a))
    pol = RandomDiscrete(6, rng=tc.SEED)
    got = [pol.select_action(np.zeros(6)) for _ in range(7)]
    assert got == [int(draw_bounded(tc.SEED, 0, c, 0, STREAM_POLICY, 6)) for c in range(7)]
    assert pol.select_action(np.zeros(6), k=0xAAAAAAAB) == 4
    batch = RandomDiscrete(5, rng=tc.SEED).select_action(np.zeros((9, 5))).cpu().numpy()
    assert np.array_equal(batch, [int(draw_bounded(tc.SEED, i, 0, 0, STREAM_POLICY, 5)) for i in range(9)])
    ex = ExclusiveEpsilonGreedy(0.3, rng=tc.SEED)
    v = np.array([0.5, 1.5, 1.5, -1.0], dtype=np.float32)
    assert np.array_equal(ex.get_action_probs(v), tc.exclusive_probs(v, 0.3))
    m = np.array([1, 0, 1, 1], dtype=bool)
    assert np.array_equal(ex.get_action_probs(v, m), tc.exclusive_probs(v, 0.3, m))
    assert ex.select_action(v, u=0.0) == 0 and ex.select_action(v, u=0.99) == 3
    mine = [ex.select_action(v) for _ in range(5)]
    want = [int(np.searchsorted(tc.cdf_of(tc.exclusive_probs(v, 0.3)),
                                float(draw_double(tc.SEED, 0, c, 0, STREAM_POLICY)), side='right'))
            for c in range(5)]
    assert mine == want
    rows = np.array([[0.0, 0.0, 1.0], [2.0, 1.0, 2.0]], dtype=np.float32)
    per_row = ExclusiveEpsilonGreedy(np.array([0.0, 1.0]))
    assert np.array_equal(per_row.get_action_probs(rows), [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])


def test_refusals_that_read_device_memory(torch_cuda):
    """An all-zero mask row and a bad entry of policy_params / param: COBEL_E_ARG before a launch."""
    from cobel_amd import _lib
    with pytest.raises(AssertionError, match='masks all actions of row 1'):
        select_n(torch_cuda, _lib.POLICY_SOFTMAX, np.zeros((2, 4)), [0xF, 0x10], [0.5, 0.5], None, [1.0], 4)
    with pytest.raises(AssertionError, match='beta -2 is not positive'):
        select_n(torch_cuda, _lib.POLICY_SOFTMAX, np.zeros((2, 4)), None, [0.5, 0.5], None, [1.0, -2.0], 4)
    with pytest.raises(AssertionError, match='epsilon 1.5 outside'):
        select_n(torch_cuda, _lib.POLICY_EXCLUSIVE, np.zeros((1, 4)), None, [0.5], None, [1.5], 4)
    env = tc.device_env('grid4', 2)
    ag = tc.device_agent(env, 'q', (tc.SOFTMAX, 2.0))
    ag.mask_actions = True
    ag._mask_bits = lambda: torch_cuda.zeros(16, dtype=torch_cuda.uint8, device='cuda')
    with pytest.raises(AssertionError, match='masks all actions of state 0'):
        ag.train(env, 1, 3, 2)
    assert int(ag._q.abs().sum().item()) == 0
    env2 = tc.device_env('grid4', 2)
    ag2 = tc.device_agent(env2, 'q', (tc.SOFTMAX, 2.0))
    ag2.policy.beta = np.array([1.0, -1.0])       # (past the constructor's assertion)
    with pytest.raises(AssertionError, match='beta -1 is not positive'):
        ag2.train(env2, 1, 3, 2)
    assert int(ag2._q.abs().sum().item()) == 0


# -- (d) frames and untouched inputs -----------------------------------------------------------------------------
def framed_session(torch, agent, kind, framed, frozen=(1, 4)):
    """A masked training session of six instances with per-instance parameters, two of them frozen
    (their trial count is at the target already), plain or inside sentinel frames."""
    from cobel_amd import _lib
    n, trials, steps, batch = 6, 3, 9, 8
    env = tc.device_env('grid4', n, base=5)
    par = None if kind == tc.RANDOM else (1.0 + 0.5 * np.arange(n) if kind == tc.SOFTMAX
                                          else 0.1 * np.arange(n))
    mask = tc.two_action_mask(np.zeros((16, 4)))
    ag = tc.device_agent(env, agent, (kind, par), alpha=0.5 + 0.05 * np.arange(n), mask=mask)
    ag._bind(env)
    ag._env_in(env)
    pol = ag.policy
    flags = _lib.F_LEARN | _lib.F_MASK_ACTIONS | ag._policy_in(pol, env, False)
    ag.monitors.reserve(trials, n, True)
    if agent == 'q':
        ag.reserve_replay(trials * steps)
    ag.describe_launch(env, pol, flags, trials, steps, 0, batch)       # (builds the parameter sets)
    ag.inst[list(frozen), _lib.I_TRIAL] = trials
    before = {'q': ag._q.clone(), 'inst': ag.inst.clone()}
    frames = None
    if framed:
        frames = fc.Frames()
        fc.swap_fused(frames, ag)
        frames.swap(ag, '_q', fc.BIG)
        frames.swap(ag, 'batches_done', fc.MARK)
        if agent == 'dynaq':
            frames.swap(ag.M, 'table', fc.MODEL_POISON)
            frames.swap(ag.M, 'index', fc.INDEX_POISON)
        else:
            frames.swap(ag, '_log', fc.log_poison(4))
        fc.frame_mask(frames, ag)
        key, sets, index, count, ppar = ag._ppol
        holder = {'sets': sets, 'index': index, 'ppar': ppar}
        frames.swap(holder, 'sets', 0)
        frames.swap(holder, 'index', 0)
        frames.swap(holder, 'ppar', 0.5)
        ag._ppol = (key, holder['sets'], holder['index'], count, holder['ppar'])
    for budget in (5, 0):
        ag._launch(env, pol, flags, trials, steps, budget, batch)
    torch.cuda.synchronize()
    out = {'q': ag._q, 'inst': ag.inst, 'batches_done': ag.batches_done}
    if agent == 'dynaq':
        out.update(model=ag.M.table, index=ag.M.index)
    else:
        out['log'] = ag._log
    for k, v in fc.monitor_arrays(ag.monitors).items():
        out[k] = v.sum(dim=0) if k[4:] in ag.monitors._PER_TRIAL else v
    return {k: v.clone() for k, v in out.items()}, before, frames


@pytest.mark.parametrize('agent,kind', [('q', tc.SOFTMAX), ('dynaq', tc.SOFTMAX), ('dynaq', tc.EXCLUSIVE),
                                        ('q', tc.RANDOM)])
def test_frames_and_frozen_instances(torch_cuda, agent, kind):
    """Sentinel frames around every table of a run: no guard byte changes, the framed run equals the
    plain one bit for bit; instances whose trials are done keep their tables and their state."""
    from cobel_amd import _lib
    plain, before, _ = framed_session(torch_cuda, agent, kind, False)
    framed, _, frames = framed_session(torch_cuda, agent, kind, True)
    frames.check()
    fc.assert_same(plain, framed)
    for k in (1, 4):
        assert torch_cuda.equal(plain['q'][k], before['q'][k]), 'a frozen instance learnt'
        assert torch_cuda.equal(plain['inst'][k], before['inst'][k]), 'a frozen instance moved'
    live = [0, 2, 3, 5]
    assert (plain['inst'][live, _lib.I_TRIAL] == 3).all()
    assert (plain['inst'][live, _lib.I_STEPS_LO] > 0).all(), 'a live instance did not move'
    if kind != tc.RANDOM:      # (three short trials of random steps need not meet the goal)
        assert plain['q'][live].abs().sum() > 0


# -- (e) what fails without the feature ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['q_soft05', 'dynaq_soft05'])
def test_agents_train_with_a_softmax_policy(torch_cuda, Z, name):
    """``QAgent(..., Softmax(beta)).train(Gridworld...)`` and the DynaQ twin complete and leave the
    reference's tables (before this kernel: an AttributeError on ``pol.epsilon``)."""
    from cobel_amd.agent import DynaQ, QAgent
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc import gridworld_tools
    from cobel_amd.policy import ExclusiveEpsilonGreedy, RandomDiscrete, Softmax  # noqa: F401
    c = tc.case(name)
    env = Gridworld(tc.grid4(gridworld_tools), n_envs=1, seed=tc.SEED, instance_base=c['inst'])
    cls = DynaQ if c['agent'] == 'dynaq' else QAgent
    ag = cls(env.observation_space, env.action_space, Softmax(c['policy'][1]))
    ag.train(env, tc.TRIALS, tc.STEPS, c['batch'])
    assert np.array_equal(np.asarray(ag.Q, dtype=np.float32), Z[name + '/Q'])
    assert ag.env_steps() == len(Z[name + '/state'])
    with pytest.raises(NotImplementedError, match='rollout records sessions that select with'):
        ag.rollout(env, 2, 5)
    if name == 'q_soft05':      # agents with kernels of their own do not take it for EpsilonGreedy
        from cobel_amd.agent import SR
        sr = SR(env.observation_space, env.action_space, ExclusiveEpsilonGreedy(0.1))
        with pytest.raises(NotImplementedError, match='served for QAgent and DynaQ'):
            sr.train(env, 1, 3)


# -- (f) the epsilon-greedy path has not moved --------------------------------------------------------------------
def test_epsilon_greedy_runs_take_the_kernels_they_took(torch_cuda):
    """describe_launch of an EpsilonGreedy run answers what tests/golden/tab_routing.json recorded
    for the shape before this kernel existed: four actions at 32 x 32 (Dyna-Q with its digest: all
    four numbers), six actions, batch 0."""
    import json
    from cobel_amd import _lib
    from cobel_amd.agent import DynaQ, QAgent
    from cobel_amd.interface import Gridworld, Topology
    from cobel_amd.misc import gridworld_tools, topology_tools
    from cobel_amd.policy import EpsilonGreedy
    with open(os.path.join(GOLDEN, 'tab_routing.json')) as f:
        table = json.load(f)
    rows = {r['name']: r['out'] for r in table['rows']}
    d = table['defaults']
    how = (_lib.F_LEARN, d['trials_target'], d['steps_per_trial'], d['step_budget'])
    keys = ('kernel', 'lds_bytes', 'workgroups_per_cu', 'instances_per_workgroup')
    env = Gridworld(gridworld_tools.make_open_field(32, 32, 0, 1), n_envs=d['n'], seed=tc.SEED)
    ag = DynaQ(env.observation_space, env.action_space, EpsilonGreedy(0.1))
    ag._bind(env)
    what = ag.describe_launch(env, ag.policy, *how, d['batch'])
    assert [what[k] for k in keys] == rows['s1024_a4_w1/dyna_b32_midx'] and set(what) == set(keys)
    assert what['kernel'] == _lib.TAB_KERNEL_PWG
    what = ag.describe_launch(env, ag.policy, *how, 0)
    assert [what[k] for k in keys] == rows['s1024_a4_w1/dyna_b0_midx']
    del ag
    qa = QAgent(env.observation_space, env.action_space, EpsilonGreedy(0.1))
    qa._bind(env)
    what = qa.describe_launch(env, qa.policy, *how, 0)
    assert [what[k] for k in keys] == rows['s1024_a4_w1/q_b0']
    nodes, starts = topology_tools.hexagonal(5, (0.0, 2.0), 3.0, '7')
    henv = Topology(nodes, starts, n_envs=d['n'], seed=tc.SEED)
    hq = QAgent(henv.observation_space, henv.action_space, EpsilonGreedy(0.1))
    hq._bind(henv)
    hq.reserve_replay(64)
    what = hq.describe_launch(henv, hq.policy, *how, d['batch'])
    assert what['kernel'] == rows['s25_a6_w1/q_b32_log'][0] == _lib.TAB_KERNEL_WQN
    assert what['instances_per_workgroup'] == rows['s25_a6_w1/q_b32_log'][3]
    assert type(hq.policy) is EpsilonGreedy and C.sizeof(_lib.TabRun) == _lib.TabPolicyRun.policy.offset
