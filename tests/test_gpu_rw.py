"""GPU tests of the Rescorla-Wagner agents, the Sequence environment and the scalar policies: the
device against the traces recorded from the real reference (tests/golden/rw_traces.npz) and, bit for
bit, against the restatement (tests/rw_common.py) on the shapes where the packing of instances into
wavefronts can go wrong.  No case is left out of the strict comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rw_common as rc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rw_traces.npz')


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


def check_against_fixture(out, Z, name):
    if rc.CASES[name]['dense']:
        # the fixture holds BLAS's sums.  The device must equal the restatement bit for bit; what
        # does not depend on the last bits equals the fixture, the rest is within the bounds
        # measured for the restatement (tests/test_oracle_rw.py)
        ref = rc.restate_case(name)
        rc.assert_same_record(out, ref, what=name + ' (device vs restatement)')
        assert np.array_equal(out['W_final'], ref['W'][-1])
        rc.assert_same_record(out, Z, name + '/', what=name,
                              keys=('action', 'reward', 'end', 'steps', 'index', 'position'))
        assert np.abs(out['value'] - Z[name + '/value']).max() <= rc.DENSE_VALUE_BOUND
        assert np.abs(out['predict'] - Z[name + '/predict']).max() <= rc.DENSE_PREDICT_BOUND
        if 'W' in out:
            assert np.abs(out['W'] - Z[name + '/W']).max() <= rc.DENSE_BOUND
        assert np.abs(out['W_final'] - Z[name + '/W'][-1]).max() <= rc.DENSE_BOUND
    else:
        rc.assert_same_record(out, Z, name + '/', what=name)
        assert np.array_equal(out['W_final'], Z[name + '/W'][-1])


# -- against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(rc.CASES))
def test_one_instance_with_trial_callbacks_reproduces_the_reference(Z, name):
    """One launch per trial; W after every trial, the log keys of the reference, and ResponseMonitor
    driven as demo_rw_binary.py drives it."""
    from cobel_amd.monitor import ResponseMonitor
    c = rc.CASES[name]
    schedule, obs = c['design']()
    D = np.asarray(next(iter(obs.values()))).size
    trials = sum(t for _, t, _ in c['sessions'])
    seen = {'W': [], 'steps': [], 'trial_reward': [], 'last_action': [], 'trial': []}
    monitor = ResponseMonitor(trials)

    def code_response(logs):
        if logs['trial'] % 2 == 0:
            logs['response'] = logs.get('action', 0) == 0
        else:
            logs['response'] = logs.get('action', 0) == 1
        return logs

    def on_trial_end(logs):
        assert {'trial_reward', 'trial', 'trial_session', 'step', 'steps', 'agent'} <= set(logs)
        assert ('action' in logs) == (c['policy'] is not None)
        seen['W'].append(logs['agent'].W[0].cpu().numpy())
        seen['steps'].append(logs['steps'])
        seen['trial_reward'].append(logs['trial_reward'])
        seen['last_action'].append(logs.get('action', -1))
        seen['trial'].append(logs['trial'])

    ag, env = rc.device_run(schedule, obs, c['nb_actions'], c['overwrite'], c['policy'],
                            c['policy_test'], c['lr'], c['sessions'], instance_base=c['inst'],
                            w0=c['w0'],
                            callbacks={'on_trial_end': [code_response, monitor.update, on_trial_end]})
    out = rc.device_record(ag, env, 0, probe=rc.probe_of(D))
    out['W'] = np.array(seen['W'])
    assert seen['trial'] == list(range(trials)) and ag.current_trial == trials
    assert np.array_equal(out['steps'], seen['steps'])
    assert np.array_equal(out['trial_reward'], seen['trial_reward'])
    if c['policy'] is not None:
        assert np.array_equal(out['last_action'], seen['last_action'])
        want = np.where(np.arange(trials) % 2 == 0, Z[name + '/last_action'] == 0,
                        Z[name + '/last_action'] == 1).astype(float)
        assert np.array_equal(monitor.responses, want)
        assert np.array_equal(monitor.CRC, np.cumsum(want))
    else:
        out.pop('last_action', None)
    check_against_fixture(out, Z, name)


@pytest.mark.parametrize('name', list(rc.CASES))
def test_eight_instances_of_one_number_reproduce_the_reference(Z, name):
    """One launch per session; all eight instances draw as instance number c['inst'] and must come
    out identical, and equal to the recorded run."""
    c = rc.CASES[name]
    schedule, obs = c['design']()
    D = np.asarray(next(iter(obs.values()))).size
    ag, env = rc.device_run(schedule, obs, c['nb_actions'], c['overwrite'], c['policy'],
                            c['policy_test'], c['lr'], c['sessions'], n_envs=8,
                            instance_ids=[c['inst']] * 8, w0=c['w0'])
    for i in range(8):
        out = rc.device_record(ag, env, i, probe=rc.probe_of(D))
        if c['policy'] is None:
            out.pop('last_action', None)
        check_against_fixture(out, Z, name)
    w = ag.W.cpu().numpy()
    assert all(np.array_equal(w[0], w[i]) for i in range(8))


# -- against the restatement ----------------------------------------------------------------------
def packed_case(D, N, policy, per_instance_of=None, lr_kind='instance', nb_actions=2,
                overwrite=False, seed=0):
    rng = np.random.default_rng(100 * D + N + seed)
    schedules, obs = rc.random_design(rng, D, 2, 14, 3, nb_actions, arrays=overwrite, dense=True)
    # two schedules of different trial lengths, round-robin; train, test, train on one interface;
    # the cap of the last session cuts the three-step trials
    schedules[1] = [t + [rc._step('o0', 0.25)] if len(t) < 3 else t[:1] for t in schedules[1]]
    sessions = [('train', 5, 4), ('test', 3, 4), ('train', 6, 2)]
    lr = {'instance': 0.1 + 0.4 * rng.random(N), 'matrix': 0.5 * rng.random((N, D)), 'float': 0.5 / D}[lr_kind]
    if np.shape(lr) == (D,):
        lr = 0.5 * rng.random((N, D))
    per_instance = per_instance_of(rng, N) if per_instance_of else None
    w0 = rng.random((N, D)) / D
    ids = 7 + 3 * np.arange(N)       # distinct instance numbers
    ag, env = rc.device_run(schedules, obs, nb_actions, overwrite, policy, None, lr, sessions,
                            n_envs=N, instance_ids=ids, w0=w0, pol_overrides=per_instance)
    rc.compare_instances(ag, env, schedules, obs, nb_actions, overwrite, policy, lr, sessions, w0,
                         ids, per_instance, what='D %d N %d' % (D, N))
    return ag, env


@pytest.mark.parametrize('N', [1, 7, 65])
@pytest.mark.parametrize('D', [1, 3, 5, 33, 64])
def test_packing_sigmoid_with_per_instance_thresholds_and_rates(D, N):
    """One lane, groups that are no power of two, a group wider than half a wave, a full wave; a
    partial last wavefront and a partial last group; dense observations."""
    ag, env = packed_case(D, N, ('sigmoid', dict(scale=3.0, value_max=D / 4 + 0.5)),
                          lambda rng, n: {'threshold': 0.2 + 0.6 * rng.random(n)})
    assert ag.env_steps() > 0 and ag.current_trial == 14
    assert (env._h_trial < 14).any(), 'the cap of the last session must hold instances back'


@pytest.mark.parametrize('D,N', [(3, 65), (33, 7)])
def test_threshold_draw_counters_diverge(D, N):
    ag, env = packed_case(D, N, ('threshold', dict(threshold=0.5, window=0.5, value_max=0.5,
                                                   code_reverse=False)), lr_kind='matrix')
    ctr = ag.policy.counter.cpu().numpy()
    assert len(set(ctr.tolist())) > 1 and 0 < ctr.max() < len(ag.recorded_steps(int(ctr.argmax())))


@pytest.mark.parametrize('D,N', [(5, 7), (64, 3)])
def test_plain_agent_with_overwritten_array_rewards(D, N):
    packed_case(D, N, None, lr_kind='float', nb_actions=3, overwrite=True)


def test_step_callbacks_equal_the_fused_run():
    c = rc.CASES['multistep_cut']
    schedule, obs = c['design']()
    seen = []

    def on_step_end(logs):
        assert {'trial_reward', 'trial', 'trial_session', 'step', 'action'} <= set(logs)
        seen.append((logs['trial'], logs['step'], logs['action'], logs['trial_reward']))

    runs = []
    for cbs in (None, {'on_step_end': [on_step_end]}):
        ag, env = rc.device_run(schedule, obs, 2, False, ('sigmoid', dict(scale=2.0)), None, 0.4,
                                c['sessions'], instance_base=31, w0=0.5, callbacks=cbs)
        runs.append(rc.device_record(ag, env, 0, probe=np.eye(3)))
    rc.assert_same_record(runs[1], {k: v for k, v in runs[0].items()}, what='per step')
    assert np.array_equal(runs[0]['W_final'], runs[1]['W_final'])
    assert len(seen) == len(runs[0]['value'])
    assert [s[2] for s in seen] == runs[0]['action'].tolist()


def test_predict_on_batch_before_training_and_after():
    from cobel_amd.agent import RescorlaWagner
    from cobel_amd.spaces import Box
    ag = RescorlaWagner(Box(0.0, 1.0, (4,)))
    ag.W.fill(0.5)
    assert np.array_equal(ag.predict_on_batch(np.eye(4)), np.full(4, 0.5))     # as the demo prints
    for D in (3, 33):
        rng = np.random.default_rng(D)
        batch, w = rng.random((5, D)), rng.normal(size=(7, D))
        ag = RescorlaWagner(Box(0.0, 1.0, (D,)))
        ag._bind_to(7, 'cuda')
        ag.W = w
        got = ag.predict_on_batch(batch).cpu().numpy()
        assert got.shape == (7, 5)
        assert np.array_equal(got, np.array([[rc.tree_dot(w[i], b) for b in batch] for i in range(7)]))


def _compare_step(env, refs, act):
    o, r, end, trunc, info = env.step(act)
    res = [ref.step(int(a)) for ref, a in zip(refs, act)]
    n = len(refs)
    flat = o.cpu().numpy().reshape(n, -1)
    assert np.array_equal(flat, np.array([x[0] for x in res]))
    assert np.array_equal(r.cpu().numpy(), np.array([x[1] for x in res]))
    assert np.array_equal(end.cpu().numpy(), np.array([x[2] for x in res]))
    assert np.array_equal(trunc.cpu().numpy(), end.cpu().numpy())
    assert np.array_equal(info['action'].cpu().numpy(), act)
    assert np.array_equal(info['step_action'].cpu().numpy(),
                          np.array([-1 if x[4]['step_action'] is None else x[4]['step_action']
                                    for x in res]))
    for x, row in zip(res, flat):
        assert not x[2] or not row.any(), 'the zero observation at a trial\'s end'
    assert np.array_equal(env.current_trial.cpu().numpy(), [ref.current_trial for ref in refs])
    assert np.array_equal(env.current_step.cpu().numpy(), [ref.current_step for ref in refs])
    assert np.array_equal(env._h_trial, [ref.current_trial for ref in refs])
    assert np.array_equal(env._h_step, [ref.current_step for ref in refs])
    return [x[2] for x in res]


def test_step_and_reset_by_hand():
    """Sequence.step() / reset() for four instances against the restatement.  Every schedule is
    stepped through to the end of each of its trials (four instances on one schedule end together,
    with different actions and so different rewards); one trial per schedule is left early and
    replayed from its first step; then both schedules side by side, round-robin, for as long as no
    instance has ended its trial."""
    from cobel_amd.interface import Sequence
    from cobel_amd.spaces import Box
    rng = np.random.default_rng(4)
    schedules, obs = rc.random_design(rng, 6, 2, 6, 4, 3, arrays=True, dense=True)
    schedules[0][2] = schedules[0][2][:1] * 3        # trials of several steps in both schedules
    schedules[1][2] = schedules[1][2][:1] * 4
    obs = {k: v.reshape(2, 3) for k, v in obs.items()}
    box = Box(0.0, 1.0, (2, 3))
    lengths = set()
    for s in (0, 1):
        env = Sequence(schedules, obs, box, 3, True, n_envs=4, seed=1, schedule_of=[s] * 4)
        refs = [rc.RefSequence(schedules[s], obs, 3, True) for _ in range(4)]
        assert not env.current_observation.any()
        left_early = False
        while refs[0].current_trial < 6:
            o, info = env.reset()
            want = [r.reset()[0] for r in refs]
            assert info == {} and o.shape == (4, 2, 3)
            assert np.array_equal(o.cpu().numpy().reshape(4, 6), np.array(want))
            length = len(schedules[s][refs[0].current_trial])
            lengths.add(length)
            for step in range(length):
                if length >= 3 and step == 1 and not left_early:
                    left_early = True        # reset() rewinds the step alone: the trial is replayed
                    break
                ended = _compare_step(env, refs, rng.integers(0, 3, 4))
                assert all(ended) == (step == length - 1) and (all(ended) or not any(ended))
        assert left_early
        with pytest.raises(IndexError, match='past the last of the 6 trials'):
            env.reset()
    assert max(lengths) >= 3 and min(lengths) == 1
    # both schedules in one interface
    env = Sequence(schedules, obs, box, 3, True, n_envs=4, seed=1)
    refs = [rc.RefSequence(schedules[i % 2], obs, 3, True) for i in range(4)]
    for _ in range(6):
        o, _ = env.reset()
        assert np.array_equal(o.cpu().numpy().reshape(4, 6), np.array([r.reset()[0] for r in refs]))
        while not any(_compare_step(env, refs, rng.integers(0, 3, 4))):
            pass
        if max(ref.current_trial for ref in refs) >= 6:
            break
    # one instance: the reference's return tuple
    one = Sequence(schedules[0], obs, box, 3, True, seed=1)
    ref = rc.RefSequence(schedules[0], obs, 3, True)
    o, _ = one.reset()
    assert type(o) is np.ndarray and o.shape == (2, 3) and np.array_equal(o.reshape(-1), ref.reset()[0])
    got, want = one.step(2), ref.step(2)
    assert np.array_equal(got[0].reshape(-1), want[0]) and got[1:] == want[1:]
    assert type(got[1]) is float and type(got[2]) is bool
    assert (one.current_trial, one.current_step) == (ref.current_trial, ref.current_step)


def test_step_refuses_an_action_outside_an_array_reward():
    """The reference indexes an array reward with the action (sequence.py:165): out of range is
    its IndexError, for one instance and for a tensor of actions; a negative one counts from the
    end."""
    from cobel_amd.interface import Sequence
    from cobel_amd.spaces import Box
    obs = {'A': np.array([1.0, 0.0])}
    trials = [[rc._step('A', np.array([0.25, 0.5, 0.75])), rc._step('A', 1.0)]] * 2
    for n in (1, 3):
        env = Sequence(trials, obs, Box(0.0, 1.0, (2,)), 3, n_envs=n, seed=1)
        env.reset()
        bad = 3 if n == 1 else np.array([0, 3, 1])
        with pytest.raises(IndexError, match='index 3 is out of bounds for axis 0 with size 3'):
            env.step(bad)
        assert not env._h_step.any()                 # nothing was launched
        out = env.step(-1 if n == 1 else np.array([-1, 0, -3]))
        if n == 1:
            assert out[1] == 0.75 and out[4]['action'] == -1
        else:
            assert out[1].cpu().numpy().tolist() == [0.75, 0.25, 0.25]
            assert out[4]['action'].cpu().numpy().tolist() == [-1, 0, -3]
        env.step(7 if n == 1 else np.array([7, -9, 5]))      # a float reward is not indexed


def test_fuzz_slice():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import fuzz_rw
    for seed in range(20):
        print(fuzz_rw.run_case(seed))
