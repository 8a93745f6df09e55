"""The ADQN agent on the device (cobel_adqn_step + cobel_mlp_fit, and the PyTorch-ROCm path) against
the traces recorded from the real reference (tests/golden/adqn_traces.npz) and the NumPy restatement
of tests/adqn_common.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adqn_common as ac  # noqa: E402
import mlp_common as mc  # noqa: E402
import mlp_gpu_common as mg  # noqa: E402
from oracle.philox import TapeRNG  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adqn_traces.npz')
# the float64 kernel against the float64 restatement: what tests/test_gpu_mlp_edges.py allows
# cobel_mlp_fit (mlp_gpu_common.agree)
RTOL, ATOL = 1e-9, 1e-12
DISCRETE = tuple(k for k in ac.EXACT if k != 'count')


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


_RUNS = {}


def fused_run(name):
    """One fused float64 run of a golden case, shared; not to be written to."""
    if name not in _RUNS:
        ag, env = ac.device_case(name, instance_base=ac.CASES[name]['inst'])
        _RUNS[name] = (ag, env, ac.device_record(ag, env))
    return _RUNS[name]


def close(got, ref, what, extra=0.0):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    worst = float(np.abs(got - ref).max()) if got.size else 0.0
    assert (np.abs(got - ref) <= extra + ATOL + RTOL * np.abs(ref)).all(), (what, worst)
    return worst


@pytest.mark.parametrize('name', sorted(ac.CASES))
def test_fused_float64_against_reference_and_restatement(Z, name):
    """Indices, rewards, end flags, states, reinforcements, draw counts and positions equal the
    reference's and the restatement's; values, errors, priorities, weights and predictions are
    within rtol 1e-9 / atol 1e-12 of the restatement, and within that plus VALUE_BOUND of the
    reference."""
    ag, env, out = fused_run(name)
    steps = len(out['value'])
    assert ag.fused_steps == int((out['idx'][:, 0] >= 0).sum()) > 0 and ag.env_steps() == steps
    ref = ac.restated(name)
    ac.assert_same_record(out, ref, what=name + ' (device vs restatement)', keys=DISCRETE)
    ac.assert_same_record(out, Z, name + '/', what=name + ' (device vs reference)', keys=DISCRETE)
    assert out['adam_steps'] == ref['adam_steps']
    for k in ('value', 'errors', 'priorities', 'weights', 'predict'):
        a = close(out[k], ref[k], (name, k, 'restatement'))
        b = close(out[k], Z[name + '/' + k], (name, k, 'reference'), ac.VALUE_BOUND)
        print('%s %s: largest difference %.3g (restatement) %.3g (reference)' % (name, k, a, b))
    # the user's model holds instance 0's trained weights
    assert ag._net.matches(ag.model, 0)


def test_torch_path_on_the_fused_shape(Z):
    """fused_loop = False: the same case through StackedTorchNetwork.train_on_device."""
    name = 'multistep_cut'
    ag, env = ac.device_case(name, instance_base=ac.CASES[name]['inst'], fused=False)
    out, ref = ac.device_record(ag, env), ac.restated(name)
    assert ag.fused_steps == 0
    ac.assert_same_record(out, ref, what=name, keys=DISCRETE)
    ac.assert_same_record(out, Z, name + '/', what=name, keys=DISCRETE)
    for k in ('value', 'errors', 'priorities', 'weights', 'predict'):
        close(out[k], ref[k], (name, k))


def _t32_session(params, idx_rows, schedule, obs, seq_actions, overwrite, sessions):
    """torch's float32 on the CPU through the same sessions, the batches being the restatement's
    (rpe off: the indices do not depend on the values)."""
    env = ac.RefSequence(schedule, obs, seq_actions, overwrite)
    net = {'p': {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in params.items()}}
    net['m'] = {k: torch.zeros_like(v) for k, v in net['p'].items()}
    net['v'] = {k: torch.zeros_like(v) for k, v in net['p'].items()}
    net['steps'] = 0.0
    states, rewards, values, at = [], [], [], 0
    for s in sessions:
        learn = s[0] == 'train'
        for _ in range(s[1]):
            state, _ = env.reset()
            for _ in range(s[2]):
                x = torch.tensor([state], dtype=torch.float32)
                with torch.no_grad():
                    value = float(mg._t32_forward(torch, net['p'], x)[0, 0])
                ns, reward, end, _, _ = env.step(value)
                values.append(value)
                if learn:
                    states.append(state)
                    rewards.append(reward)
                    idx = idx_rows[at]
                    bx = torch.tensor(np.array(states)[idx], dtype=torch.float32)
                    by = torch.tensor(np.array(rewards)[idx], dtype=torch.float32)[:, None]
                    for _ in range(s[4]):
                        net = mg._t32_fit_step(torch, net, bx, by, None, True, ac.HYPER)
                at += 1
                state = ns
                if end:
                    break
    return np.array(values), ac.weights_of({k: v.numpy() for k, v in net['p'].items()})


def test_fused_float32_against_the_restatement():
    """One float32 case, rpe off so that the drawn indices do not depend on the values.  The bound
    is formed as for cobel_mlp_fit in float32 (docs/MEASUREMENTS.md section 14): torch's float32 on
    the CPU runs the same sessions on the same batches, and the kernel may differ from the float64
    restatement by F32_FACTOR times what torch differs by, at least F32_FLOOR (mc.f32_bound)."""
    c = ac.CASES['unit_no_rpe']
    schedule, obs, seq_actions = c['design']()
    sessions = [('train', 10, 10, 32, 1), ('test', 4, 10)]
    stack = mc.draw_networks(np.random.default_rng(77), 1, 2, 1, np.float32)
    params = mc.one(stack, 0)
    ref = ac.restate(schedule, obs, c['overwrite'], seq_actions, params, 0.9, False, sessions, 21,
                     ac.BATCH)
    ag, env = ac.device_run(schedule, obs, c['overwrite'], seq_actions, params, 0.9, False, sessions,
                            instance_base=21, dtype=np.float32)
    out = ac.device_record(ag, env)
    assert ag.dtype == torch.float32 and ag.fused_steps == 10
    ac.assert_same_record(out, ref, what='float32', keys=DISCRETE + ('priorities',))
    t_values, t_weights = _t32_session(params, ref['idx'], schedule, obs, seq_actions,
                                       c['overwrite'], sessions)
    for k, yard in (('value', t_values), ('weights', t_weights)):
        kernel, torch_err = mc.rel_err(out[k], ref[k]), mc.rel_err(yard, ref[k])
        print('float32 %s: kernel %.3e torch %.3e' % (k, kernel, torch_err))
        assert torch_err <= mg.YARD_CAP_FIT, (k, torch_err)
        assert kernel <= mc.f32_bound(torch_err), (k, kernel, torch_err)
    # errors = value - reward in float64 from the float32 value, widened exactly
    assert np.array_equal(out['errors'], out['value'][:10].astype(np.float32).astype(np.float64)
                          - out['reward'][:10])


class UnitModel(torch.nn.Module):
    """unit_tests/test_adqn.py: Linear(2, 32)-ReLU-Linear(32, 1) in float64."""

    def __init__(self):
        super().__init__()
        self.hidden = torch.nn.Linear(2, 32)
        self.output = torch.nn.Linear(32, 1)
        self.double()

    def forward(self, x):
        return self.output(torch.nn.functional.relu(self.hidden(x)))


def test_torch_path_on_the_reference_unit_test_network():
    """A network cobel_mlp_fit does not cover, and a batch of 20: the memory kernel still stores
    and draws, torch trains.  Against the same loop on the CPU (torch float64, torch.optim.Adam,
    MSE with mean reduction) around the restated memory."""
    import copy
    c = ac.CASES['unit']
    schedule, obs, seq_actions = c['design']()
    torch.manual_seed(5)
    proto = UnitModel()
    sessions, B = [('train', 10, 10, 20, 2), ('test', 10, 10)], 20
    cpu = copy.deepcopy(proto)
    opt = torch.optim.Adam(cpu.parameters())
    env = ac.RefSequence(schedule, obs, seq_actions, False)
    mem = ac.RefMemory(2, 1.0, True, TapeRNG(ac.SEED, 33, ac.STREAM_ADQN_MEMORY))
    values, idxs = [], []
    for s in sessions:
        for _ in range(s[1]):
            state, _ = env.reset()
            with torch.no_grad():
                value = float(cpu(torch.tensor([state], dtype=torch.float64))[0, 0])
            _, reward, _, _, _ = env.step(value)
            values.append(value)
            if s[0] == 'train':
                mem.store(state, value, reward)
                idx = mem.sample(B)
                idxs.append(idx)
                for _ in range(s[4]):
                    opt.zero_grad()
                    pred = cpu(torch.from_numpy(mem.states[idx]))
                    ((pred - torch.from_numpy(mem.reinforcements[idx])[:, None]) ** 2).mean().backward()
                    opt.step()
    assert mem.margin > 1e-9
    ag, denv = ac.device_run(schedule, obs, False, seq_actions, None, 1.0, True, sessions,
                             instance_base=33, model=proto)
    assert ag.fused_steps == 0 and ag._net._mlp3_names() is None
    rows = ag.recorded_steps(0)
    assert np.array_equal(ag.recorded_indices(0)[:10], np.array(idxs))
    assert (ag.recorded_indices(0)[10:] == -1).all()
    close(rows[:, 0], np.array(values), 'values')
    for got, want in zip(ag._net.get_weights(0), cpu.state_dict().values()):
        close(got, want.numpy(), 'weights')
    assert ag.memory.count == 10 and np.array_equal(ag.memory.reinforcements, mem.reinforcements)
    close(ag.memory.priorities, mem.priorities, 'priorities')
    assert ag.retrieve_v(np.array([1.0, 0.0])).shape == (1,)
    assert ag.predict_on_batch(np.eye(2)).shape == (2, 1)


def _rotated(schedule, k):
    return schedule[k:] + schedule[:k]


def test_instances_depend_on_their_instance_number_only():
    """Three instances in one run — two schedules whose trial lengths differ, so the instances hold
    different counts — against three single runs with the same instance numbers: bit-equal."""
    c = ac.CASES['multistep_cut']
    schedule, obs, seq_actions = c['design']()
    schedules = [schedule, _rotated(schedule, 2)]
    params, ids, of = ac.case_params('multistep_cut'), [5, 900, 17], [0, 1, 1]
    sessions = [('train', 6, 2, 32, 1), ('train', 5, 5, 32, 2), ('test', 2, 5)]
    ag, env = ac.device_run(schedules, obs, True, seq_actions, params, 0.9, True, sessions, n_envs=3,
                            instance_ids=ids, schedule_of=of)
    counts = ag.memory._h_count.tolist()
    assert len(set(counts)) > 1 and mg._host(ag.memory.count).tolist() == counts
    assert tuple(ag.memory.states.shape) == (3, max(counts), 3)
    for j in range(3):
        one, env1 = ac.device_run(schedules[of[j]], obs, True, seq_actions, params, 0.9, True,
                                  sessions, instance_base=ids[j])
        a, b = ac.device_record(ag, env, j), ac.device_record(one, env1)
        for k in a:
            assert np.array_equal(a[k], b[k]), (j, k)
    # instance 0 is the golden case's own instance and design: its first session is the fixture's
    ref, got = ac.restated('multistep_cut'), ac.device_record(ag, env, 0)
    first = int((ref['steps'][:6] + 1).sum())
    assert np.array_equal(got['idx'][:first], ref['idx'][:first])
    close(got['value'][:first], ref['value'][:first], 'first session')


def test_two_sessions_equal_one_and_cross_a_capacity_growth():
    c = ac.CASES['two_sessions']
    schedule, obs, seq_actions = c['design']()
    params = ac.case_params('two_sessions')
    ag2, env2, two = fused_run('two_sessions')
    assert ag2.memory.cap == 32          # 16 after the first session's reservation, then doubled
    ag1, env1 = ac.device_run(schedule, obs, False, seq_actions, params, c['decay'], c['rpe'],
                              [('train', 20, 10, 32, 1)], instance_base=c['inst'])
    one = ac.device_record(ag1, env1)
    for k in two:
        assert np.array_equal(two[k], one[k]), k


def test_test_leaves_memory_and_weights_untouched():
    c = ac.CASES['unit_decay']
    schedule, obs, seq_actions = c['design']()
    ag, env = ac.device_run(schedule, obs, False, seq_actions, ac.case_params('unit_decay'),
                            c['decay'], c['rpe'], [('train', 10, 10, 32, 1)], instance_base=1)
    before = ac.device_record(ag, env)
    ag.test(env, 10, 10)
    after = ac.device_record(ag, env)
    for k in ('states', 'reinforcements', 'errors', 'priorities', 'weights', 'predict', 'draws',
              'adam_steps'):
        assert np.array_equal(before[k], after[k]), k
    assert len(after['value']) == 20 and (after['idx'][10:] == -1).all()
    assert ag.current_trial == 20 and after['position'].tolist() == [20, 1]
    with pytest.raises(IndexError, match='list index out of range'):
        ag.test(env, 1, 10)
    assert ag.current_trial == 20


def test_logs_and_callbacks():
    """One instance with step and trial callbacks: the reference's log keys, the same results as
    without callbacks, ``stop`` ends the session after the trial."""
    name = 'multistep_cut'
    c = ac.CASES[name]
    schedule, obs, seq_actions = c['design']()
    seen = {'trial_begin': [], 'step_begin': [], 'step_end': [], 'trial_end': []}
    hooks = {'on_' + k: [lambda logs, k=k: seen[k].append(dict(logs))] for k in seen}
    ag, env = ac.device_case(name, instance_base=c['inst'], callbacks=hooks)
    out, plain = ac.device_record(ag, env), fused_run(name)[2]
    for k in out:
        assert np.array_equal(out[k], plain[k]), k
    trials = sum(s[1] for s in c['sessions'])
    steps = len(out['value'])
    assert [len(seen[k]) for k in ('trial_begin', 'step_begin', 'step_end', 'trial_end')] == \
        [trials, steps, steps, trials]
    assert [l['trial'] for l in seen['trial_end']] == list(range(trials))
    assert [l['trial_session'] for l in seen['trial_begin']] == \
        [k for s in c['sessions'] for k in range(s[1])]
    assert [l['steps'] for l in seen['trial_end']] == out['steps'].tolist()
    assert [l['step'] for l in seen['trial_end']] == out['steps'].tolist()
    assert np.array_equal([l['trial_reward'] for l in seen['trial_end']], out['trial_reward'])
    for i, l in enumerate(seen['step_end']):
        assert set(l) >= {'trial_reward', 'trial', 'trial_session', 'step', 'state', 'action',
                          'reward', 'next_state', 'terminal', 'agent'}
        assert l['action'] == out['value'][i] and l['reward'] == out['reward'][i]
        assert l['terminal'] == 1 - int(out['end'][i]) and l['agent'] is ag
        assert l['state'].shape == (3,) and (l['terminal'] == 1 or not l['next_state'].any())
    learned = out['idx'][:, 0] >= 0
    assert np.array_equal(np.array([l['state'] for l in seen['step_end']])[learned], out['states'])
    assert 'steps' not in seen['step_end'][0] and 'step' not in seen['trial_begin'][0]

    # many instances: the trial hooks fire per session with the means over the instances
    ends = []
    agn, envn = ac.device_run(schedule, obs, True, seq_actions, ac.case_params(name), 0.9, True,
                              [('train', 4, 5, 32, 1)], n_envs=2, instance_base=c['inst'],
                              callbacks={'on_trial_end': [lambda logs: ends.append(dict(logs))]})
    assert [l['trial'] for l in ends] == [0, 1, 2, 3] and all(l['count'] == 2 for l in ends)
    assert np.allclose([l['trial_reward'] for l in ends],
                       mg._host(agn.trial_reward_trace[:, :4]).mean(axis=0))

    def stop(logs):
        logs['agent'].stop = logs['trial'] == 2

    ags, envs = ac.device_run(schedule, obs, True, seq_actions, ac.case_params(name), 0.9, True,
                              [('train', 6, 5, 32, 1)], instance_base=c['inst'],
                              callbacks={'on_trial_end': [stop]})
    assert ags.current_trial == 3 and envs.current_trial == 3
    assert ags.memory.count == int(ags._trace_len[0].item()) == 2 + 1 + 3
