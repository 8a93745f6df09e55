"""GPU tests of the AssociativeNetwork agent: the device against the traces recorded from the real
reference (tests/golden/anet_traces.npz) and, bit for bit, against the restatement
(tests/anet_common.py) on the shapes where the packing of instances into wavefronts can go wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anet_common as ac  # noqa: E402
import rw_common as rc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'anet_traces.npz')
LOG_KEYS = {'trial_reward', 'trial', 'trial_session', 'step', 'steps', 'state', 'action', 'reward',
            'next_state', 'terminal', 'agent'}


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


def check_against_fixture(out, Z, name):
    """Bit-equal to the restatement in every case; bit-equal to the reference in the sparse cases,
    within the bounds measured for the restatement (tests/test_oracle_anet.py) in the dense one."""
    ref = ac.restated(name)
    ac.assert_same_record(out, ref, what=name + ' (device vs restatement)')
    assert np.array_equal(out['We_final'], ref['We'][-1]) and np.array_equal(out['Wi_final'], ref['Wi'][-1])
    if not ac.CASES[name]['dense']:
        ac.assert_same_record(out, Z, name + '/', what=name)
        assert np.array_equal(out['We_final'], Z[name + '/We'][-1])
        assert np.array_equal(out['Wi_final'], Z[name + '/Wi'][-1])
        return
    ac.assert_same_record(out, Z, name + '/', what=name, keys=ac.DISCRETE)
    assert np.abs(out['q'] - Z[name + '/q']).max() <= ac.DENSE_BOUND['q']
    assert np.abs(out['predict'] - Z[name + '/predict']).max() <= ac.DENSE_BOUND['predict']
    for k in ('We', 'Wi'):
        if k in out:
            assert np.abs(out[k] - Z[name + '/' + k]).max() <= ac.DENSE_BOUND['W']
        assert np.abs(out[k + '_final'] - Z[name + '/' + k][-1]).max() <= ac.DENSE_BOUND['W']


# -- against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ac.CASES))
def test_one_instance_with_trial_callbacks_reproduces_the_reference(Z, name):
    """One launch per trial: both matrices after every trial and the log keys of the reference."""
    c = ac.CASES[name]
    D = Z[name + '/We'].shape[1]
    trials = len(Z[name + '/steps'])
    seen = {'We': [], 'Wi': [], 'steps': [], 'trial_reward': [], 'trial': [], 'action': []}

    def on_trial_end(logs):
        assert set(logs) == LOG_KEYS
        for k in ac.KEYS:
            seen['W' + k[0]].append(logs['agent'].weights[k][0].cpu().numpy())
        for k in ('steps', 'trial_reward', 'trial', 'action'):
            seen[k].append(logs[k])

    rec = ac.new_record()
    ag, env = ac.device_case(name, instance_base=c['inst'], rec=rec,
                             callbacks={'on_trial_end': [on_trial_end]})
    out = ac.device_record(ag, env, 0, probe=ac.probe_of(D))
    out['We'], out['Wi'] = np.array(seen['We']), np.array(seen['Wi'])
    out['mid_predict'] = np.array(rec['mid_predict'], dtype=np.float64).reshape(
        (-1,) + out['We'].shape[1:])
    assert seen['trial'] == list(range(trials)) and ag.current_trial == trials
    assert np.array_equal(out['steps'], seen['steps'])
    assert np.array_equal(out['trial_reward'], seen['trial_reward'])
    # (logs['action'] at a trial's end is that of its last step)
    assert seen['action'] == out['action'][np.cumsum(out['steps'] + 1) - 1].tolist()
    check_against_fixture(out, Z, name)


@pytest.mark.parametrize('name', list(ac.CASES))
def test_eight_instances_of_one_number_reproduce_the_reference(Z, name):
    """One launch per session; all eight instances draw as instance number c['inst'] and must come
    out identical, and equal to the recorded run."""
    c = ac.CASES[name]
    D = Z[name + '/We'].shape[1]
    ag, env = ac.device_case(name, n_envs=8, instance_ids=[c['inst']] * 8)
    outs = {i: ac.device_record(ag, env, i) for i in (0, 7)}
    # (one call for all instances, after the counters were read: it advances the agent's stream)
    predict = ag.predict_on_batch(ac.probe_of(D)).cpu().numpy()
    for i, out in outs.items():
        out['predict'] = predict[i]
        check_against_fixture(out, Z, name)
    for k in ac.KEYS:
        w = ag.weights[k].cpu().numpy()
        assert all(np.array_equal(w[0], w[i]) for i in range(8))
    assert len(set(ag._agent_ctr.tolist())) == 1 and len(set(ag.policy.counter.tolist())) == 1


# -- against the restatement ----------------------------------------------------------------------
SESSIONS = [('train', 5, 4), ('test', 3, 4), ('train', 6, 2)]


def drifting_case(D, N, n_actions, seed=0):
    """Two schedules of different trial lengths, round-robin; train, test, train on one interface,
    the cap of the last session cutting the three-step trials; per-instance epsilon, saturation and
    learning rates; dense observations; array rewards under overwrite."""
    rng = np.random.default_rng(1000 * D + 10 * N + n_actions + seed)
    seq_actions = max(n_actions - 1, 2)
    schedules, obs = rc.random_design(rng, D, 2, 14, 3, seq_actions, arrays=True, dense=True)
    schedules[1] = [t + [rc._step('o0', 0.25)] if len(t) < 3 else t[:1] for t in schedules[1]]
    shape = (N, D, n_actions - 1)
    kw = dict(saturation={k: 1.0 + 4.0 * rng.random(shape) for k in ac.KEYS},
              learning_rate={k: 0.3 * rng.random(shape) for k in ac.KEYS}, noise=0.5)
    eps = 0.05 + 0.5 * rng.random(N)
    ids = 7 + 3 * np.arange(N)       # distinct instance numbers
    return schedules, obs, seq_actions, kw, eps, ids


def restate_instance(case, n_actions, i, sessions=SESSIONS, probe=None):
    schedules, obs, seq_actions, kw, eps, ids = case
    kw_i = dict(kw, saturation={k: kw['saturation'][k][i] for k in ac.KEYS},
                learning_rate={k: kw['learning_rate'][k][i] for k in ac.KEYS})
    return ac.restate(schedules[i % 2], obs, seq_actions, True, n_actions, eps[i], None, kw_i,
                      sessions, int(ids[i]), probe=probe)


def frame(t, pad=16):
    """A copy of ``t`` inside a larger buffer of sentinels: (the view, the buffer)."""
    import torch
    sentinel = float('nan') if t.dtype.is_floating_point else -77
    big = torch.full((t.numel() + 2 * pad,), sentinel, dtype=t.dtype, device=t.device)
    view = big[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, big


def frame_intact(big, n, pad=16):
    edge = np.concatenate([big[:pad].cpu().numpy(), big[pad + n:].cpu().numpy()])
    return bool(np.isnan(edge).all()) if big.dtype.is_floating_point else bool((edge == -77).all())


@pytest.mark.parametrize('D,N,n_actions', [(2, 37, 3), (64, 3, 9), (1, 65, 2), (5, 9, 4), (33, 2, 3)])
def test_packing_edges_leave_the_frames_untouched(D, N, n_actions):
    """Instance counts that leave the last wavefront partly filled (37 instances at G = 2, 3 at
    G = 64, ...), padding lanes (D = 5, 33), one lane per instance: every instance equals its
    restatement bit for bit, and the sentinels around every tensor the kernel writes stay."""
    import torch
    from cobel_amd import _lib
    from cobel_amd.agent import AssociativeNetwork
    from cobel_amd.interface import Sequence
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete
    case = drifting_case(D, N, n_actions)
    schedules, obs, seq_actions, kw, eps, ids = case
    env = Sequence(schedules, obs, Box(0.0, 1.0, (D,)), seq_actions, True, n_envs=N, seed=ac.SEED,
                   instance_ids=ids)
    ag = AssociativeNetwork(env.observation_space, Discrete(n_actions), EpsilonGreedy(eps), **kw)
    ag.record_steps = 64
    ag._bind_to(N, env.device)
    ag._reserve(14)
    ag.policy.counter = torch.zeros(N, dtype=torch.int32, device=env.device)
    frames = {}
    for k in ac.KEYS:
        ag.weights[k], frames['weights ' + k] = frame(ag.weights[k])
    for holder, names in ((ag, ('_agent_ctr', '_mid', '_trew', 'trial_reward_trace',
                                'trial_steps_trace', 'trial_action_trace', '_trace', '_trace_len')),
                          (ag.policy, ('counter',)), (env, ('_trial', '_step'))):
        for name in names:
            view, frames[name] = frame(getattr(holder, name))
            setattr(holder, name, view)
    env.seq.cur_trial, env.seq.cur_step = _lib.ptr(env._trial), _lib.ptr(env._step)
    ac.run_sessions(ag, env, SESSIONS, None)
    torch.cuda.synchronize()
    sizes = {'weights excitatory': N * D * (n_actions - 1), 'weights inhibitory': N * D * (n_actions - 1),
             '_trace': N * 64 * (2 + n_actions), 'trial_reward_trace': N * 14,
             'trial_steps_trace': N * 14, 'trial_action_trace': N * 14}
    for name, big in frames.items():
        assert frame_intact(big, sizes.get(name, N)), name
    probe = np.random.default_rng(99).random((3, D))
    for i in range(N) if N <= 9 else (0, 1, 31, 32, N - 2, N - 1):
        ref = restate_instance(case, n_actions, i, probe=probe)
        out = ac.device_record(ag, env, i, probe=None)
        ac.assert_same_record(out, ref, what='D %d N %d instance %d' % (D, N, i))
        assert np.array_equal(out['We_final'], ref['We'][-1]), i
        assert np.array_equal(out['Wi_final'], ref['Wi'][-1]), i
    p = ag.predict_on_batch(probe).cpu().numpy()
    for i in (0, N - 1):
        # (the probe of restate_instance follows the sessions, as this call does)
        assert np.array_equal(p[i], restate_instance(case, n_actions, i, probe=probe)['predict'])
    assert ag.env_steps() > 0 and ag.current_trial == 14
    assert (env._h_trial < 14).any(), 'the cap of the last session must hold instances back'


def test_drifting_instances_equal_their_single_instance_runs():
    """Seven instances share one wavefront (G = 4) on schedules of different trial lengths, each
    with its own epsilon, saturation and learning-rate rows: every one equals the run of that
    instance alone under the same instance number, and the restatement."""
    D, N, n_actions = 3, 7, 4
    case = drifting_case(D, N, n_actions, seed=5)
    schedules, obs, seq_actions, kw, eps, ids = case
    ag, env = ac.device_run(schedules, obs, seq_actions, True, n_actions, eps, None, kw, SESSIONS,
                            n_envs=N, instance_ids=ids)
    # the two schedules end their trials at different steps: the groups of the wavefront drift
    lat = ag.trial_steps_trace.cpu().numpy()
    assert len(set(env._h_trial.tolist())) > 1 and not np.array_equal(lat[0], lat[1])
    for i in range(N):
        kw_i = dict(kw, saturation={k: kw['saturation'][k][i] for k in ac.KEYS},
                    learning_rate={k: kw['learning_rate'][k][i] for k in ac.KEYS})
        one, env1 = ac.device_run(schedules[i % 2], obs, seq_actions, True, n_actions, float(eps[i]),
                                  None, kw_i, SESSIONS, instance_ids=[ids[i]])
        out, alone = ac.device_record(ag, env, i), ac.device_record(one, env1, 0)
        ac.assert_same_record(out, alone, what='instance %d vs alone' % i)
        ac.assert_same_record(out, restate_instance(case, n_actions, i), what='instance %d' % i)
        for k in ('We_final', 'Wi_final'):
            assert np.array_equal(out[k], alone[k]), (i, k)


# -- launch modes ---------------------------------------------------------------------------------
def test_trial_and_step_callbacks_equal_the_fused_run():
    name = 'multistep_cut'
    c = ac.CASES[name]
    schedule, obs, _ = c['design']()
    steps_seen, trials_seen = [], []

    def on_step_end(logs):
        assert set(logs) == LOG_KEYS - {'steps'}
        steps_seen.append((logs['trial'], logs['step'], logs['action'], logs['reward'],
                           logs['terminal'], logs['state'].copy(), logs['next_state'].copy(),
                           logs['trial_reward']))

    def on_trial_end(logs):
        assert set(logs) == LOG_KEYS
        trials_seen.append((logs['trial'], logs['steps'], logs['trial_reward'], logs['action']))

    runs = []
    for cbs in (None, {'on_trial_end': [on_trial_end]},
                {'on_step_end': [on_step_end], 'on_trial_end': [on_trial_end]}):
        ag, env = ac.device_case(name, instance_base=c['inst'], callbacks=cbs)
        runs.append(ac.device_record(ag, env, 0, probe=np.eye(3)))
    for k, out in enumerate(runs[1:]):
        ac.assert_same_record(out, runs[0], what='launch mode %d' % (k + 1))
        for key in ('We_final', 'Wi_final'):
            assert np.array_equal(out[key], runs[0][key])
    ref = runs[0]
    T = len(ref['steps'])
    assert trials_seen[:T] == trials_seen[T:]
    assert [t[1] for t in trials_seen[:T]] == ref['steps'].tolist()
    assert [t[2] for t in trials_seen[:T]] == ref['trial_reward'].tolist()
    assert len(steps_seen) == len(ref['action'])
    assert [s[2] for s in steps_seen] == ref['action'].tolist()
    assert [s[3] for s in steps_seen] == ref['reward'].tolist()
    assert [s[4] for s in steps_seen] == (1 - ref['end']).tolist()
    # state and next_state are the schedule's observations, the zero observation at a trial's end
    env = rc.RefSequence(schedule, obs, 2, True)
    at = 0
    for kind, trials, cap in c['sessions']:
        for _ in range(trials):
            state, _ = env.reset()
            for step in range(cap):
                ns, _, end, _, _ = env.step(steps_seen[at][2])
                assert steps_seen[at][1] == step
                assert steps_seen[at][5].tolist() == state and steps_seen[at][6].tolist() == ns
                assert not end or not any(ns)
                state, at = ns, at + 1
                if end:
                    break
    assert at == len(steps_seen)


# -- direct calls ---------------------------------------------------------------------------------
def test_retrieve_q_and_update_q_equal_the_steps_of_the_session_kernel():
    from cobel_amd.agent import AssociativeNetwork
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box, Discrete
    c = ac.CASES['unit_rates']
    schedule, obs, _ = c['design']()
    ag, env = ac.device_case('unit_rates', instance_base=0)
    rows = ag.recorded_steps(0)[:10]          # the training session: one step per trial
    hand = AssociativeNetwork(Box(0.0, 1.0, (2,)), Discrete(3), EpsilonGreedy(0.1), rng=ac.SEED,
                              **c['agent_kw'])
    for t, row in enumerate(rows):
        state = np.asarray(obs[schedule[t][0]['observation']])
        q = hand.retrieve_q(state)
        assert type(q) is np.ndarray and q.shape == (2,) and np.array_equal(q, row[3:])
        hand.update_q({'state': state, 'action': int(row[0]), 'reward': float(row[1]),
                       'next_state': np.zeros(2), 'terminal': 0})
    for k in ac.KEYS:      # (the test session that followed left the weights alone)
        assert ag.weights[k].any()
        assert np.array_equal(hand.weights[k][0].cpu().numpy(), ag.weights[k][0].cpu().numpy())
    assert int(hand._agent_ctr[0].item()) == 20
    # an action outside the outputs changes nothing, as the reference's all-zero action_vector
    before = {k: hand.weights[k].clone() for k in ac.KEYS}
    hand.update_q({'state': np.ones(2), 'action': 2, 'reward': 1.0})
    assert all(np.array_equal(before[k].cpu().numpy(), hand.weights[k].cpu().numpy()) for k in ac.KEYS)
    # vectorised: one experience per instance, the same observation for all
    many, envs = ac.device_case('unit_rates', n_envs=5, instance_ids=[0, 0, 3, 0, 4],
                                record=0)
    q = many.retrieve_q(np.array([1.0, 0.0]))
    assert tuple(q.shape) == (5, 2)
    q = q.cpu().numpy()
    assert np.array_equal(q[0], q[1]) and np.array_equal(q[0], q[3]) and not np.array_equal(q[0], q[2])
    w0 = {k: many.weights[k].cpu().numpy().copy() for k in ac.KEYS}
    many.update_q({'state': np.array([[1.0, 0.0]] * 4 + [[0.0, 2.0]]), 'action': [0, 1, 0, 1, 1],
                   'reward': [1.0, 1.0, -1.0, 0.0, 0.5]})
    lr, sat = c['agent_kw']['learning_rate'], 20.0
    for i, (j, a, k) in enumerate(((0, 0, 'excitatory'), (0, 1, 'excitatory'), (0, 0, 'inhibitory'),
                                   (0, 1, 'inhibitory'), (1, 1, 'excitatory'))):
        want = {key: w0[key][i].copy() for key in ac.KEYS}
        want[k][j, a] = want[k][j, a] + lr[k][j, a] * (1.0 * (sat - want[k][j, a]))
        for key in ac.KEYS:
            assert np.array_equal(many.weights[key][i].cpu().numpy(), want[key]), (i, key)


def test_a_session_split_in_two_equals_one():
    c = ac.CASES['eight_outputs']
    schedule, obs, seq_actions = c['design']()
    outs = []
    for sessions in ([('train', 24, 10)], [('train', 9, 10), ('train', 15, 10)]):
        ag, env = ac.device_run(schedule, obs, seq_actions, False, 9, c['eps'], None, c['agent_kw'],
                                sessions, n_envs=3, instance_ids=[5, 6, 5])
        outs.append([ac.device_record(ag, env, i) for i in range(3)])
    for one, two in zip(*outs):
        ac.assert_same_record(two, one, what='split session')
        assert np.array_equal(one['We_final'], two['We_final'])
        assert np.array_equal(one['Wi_final'], two['Wi_final'])
    want = ac.restated('eight_outputs')
    assert np.array_equal(outs[0][0]['We_final'], want['We'][23])
    assert np.array_equal(outs[0][2]['q'], want['q'][:24])
