"""The session driver the Sequence agents share (``SequenceAgent``, agent/agent.py), pinned once on
the host: which launches a session makes in each callback mode, what the callbacks get and when,
how the traces grow — and ``Sequence.session_steps`` / ``plan_session`` on their one walker.  The
agent here is a stub whose hooks call no library function; the Sequence lives on the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rw_common as rc  # noqa: E402

from cobel_amd import _lib  # noqa: E402
from cobel_amd.agent.agent import SequenceAgent  # noqa: E402
from cobel_amd.interface import Sequence  # noqa: E402
from cobel_amd.spaces import Box  # noqa: E402

OBS = {n: np.eye(2)[i] for i, n in enumerate('AB')}
STEPS = 2       # the cap: the first trial ends exactly on it, the last is cut by it


class HostSequence(Sequence):
    def _on_device(self) -> None:
        pass


def sequence(n_envs, lengths=(2, 1, 3), **kw):
    trials = [[rc._step('AB'[k % 2], 1.0) for k in range(n)] for n in lengths]
    return HostSequence(trials, OBS, Box(0.0, 1.0, (2,)), device='cpu', seed=1, n_envs=n_envs, **kw)


class Stub(SequenceAgent):
    """Records every hook; a launch of whole trials writes reward 10 t + i and steps t + i for trial
    t of instance i, a launch of one step the row (step, launch number, its reward, end)."""
    _who = 'Stub'
    _row_width = 4

    def __init__(self, callbacks=None) -> None:
        super().__init__(Box(0.0, 1.0, (2,)), Box(-np.inf, np.inf, (1,), np.float64), callbacks)
        self.dim = 2
        self.calls, self.rows = [], []
        self._at = self._step = None

    def train(self, interface, trials, steps=STEPS):
        self._session(interface, trials, steps, True)

    def test(self, interface, trials, steps=STEPS):
        self._session(interface, trials, steps, False)

    def predict_on_batch(self, batch):
        raise NotImplementedError

    def _bind_to(self, n_envs, device):
        if self.n_envs is None:
            self.n_envs, self.device = int(n_envs), torch.device(device)
            self._session_buffers()
            self._rec = torch.zeros(4, dtype=torch.float64)

    def _launch(self, interface, pol, learn, first, trials, steps, budget):
        self.calls.append(('run', first, trials, steps, budget))
        if budget == 0:
            for t in range(first, first + trials):
                for i in range(self.n_envs):
                    self.trial_reward_trace[i, t] = 10.0 * t + i
                    self.trial_steps_trace[i, t] = t + i
            return
        if first != self._at:
            self._at, self._step = first, 0
        k, step = len(self.rows), self._step
        row = [step, k, 0.25 * (k + 1), float(step + 1 >= int(interface.step_at(0)[1]))]
        self.rows.append(row)
        self._step += 1
        (self._step_row[0, 0] if self.one_trial_launch else self._rec)[:] = torch.tensor(row)

    def _step_logs(self, interface, step):
        value, launch, reward, end = (self._step_row[0, 0] if self.one_trial_launch
                                      else self._rec).numpy()
        self.calls.append(('step', step))
        return {'launch': int(launch)}, float(reward), end

    def _trial_logs(self, interface, at, last_step):
        return {'at': at}

    def _after_trial(self, logs=None):
        self.calls.append(('after', None if logs is None else logs['trial']))
        return logs


class StepOnlyStub(Stub):
    one_trial_launch = False      # what ADQN sets: no launch covers one trial


def recording(agent_class, *names, stop_after=None):
    """An agent whose callbacks ``names`` append (name, logs without the agent) to ``agent.calls``."""
    def hook(name):
        def call(logs):
            ag = logs['agent']
            ag.calls.append((name, {k: v for k, v in logs.items() if k != 'agent'}))
            if name == 'on_trial_end' and logs['trial_session'] + 1 == stop_after:
                ag.stop = True
        return call
    return agent_class({name: [hook(name)] for name in names})


def of(calls, kind):
    return [c[1:] if kind == 'run' else c[1] for c in calls if c[0] == kind]


def test_batched_session_is_one_run():
    env, ag = sequence(3), Stub()
    ag.train(env, 3)
    assert ag.calls == [('run', 0, 3, STEPS, 0), ('after', None)]
    assert ag.current_trial == 3 and ag._sessions == 1
    assert env._h_trial.tolist() == [2, 2, 2] and env._h_step.tolist() == [2, 2, 2]   # cut: replayed
    assert ag.trial_reward_trace.shape == ag.trial_steps_trace.shape == (3, 3)
    assert ag.trial_reward_trace.dtype == torch.float64 and ag.trial_steps_trace.dtype == torch.int32
    assert ag.trial_action_trace is None and ag._trace is None
    # a second session continues at current_trial; the traces grow and keep their columns
    before = ag.trial_reward_trace.clone()
    ag.train(env, 1, 3)
    assert ag.calls[2] == ('run', 3, 1, 3, 0) and ag.current_trial == 4
    assert ag.trial_reward_trace.shape == (3, 4) and ag.trial_steps_trace.shape == (3, 4)
    assert torch.equal(ag.trial_reward_trace[:, :3], before)
    assert env._h_trial.tolist() == [3, 3, 3]
    with pytest.raises(IndexError, match='past the last of the 3 trials'):
        ag.train(env, 1)
    assert len(ag.calls) == 4 and ag.current_trial == 4


def test_reserve_fills_with_nan_and_minus_one():
    ag = Stub()
    ag._trial_traces = lambda: ('trial_reward_trace', 'trial_steps_trace', 'trial_action_trace')
    ag.record_steps = 5
    ag._bind_to(3, 'cpu')
    ag._reserve(3)
    assert torch.isnan(ag.trial_reward_trace).all() and ag.trial_reward_trace.shape == (3, 3)
    assert (ag.trial_steps_trace == -1).all() and (ag.trial_action_trace == -1).all()
    assert ag._trace.shape == (3, 5, 4) and not ag._trace.any() and ag._trace_len.tolist() == [0] * 3
    ag.trial_steps_trace[:, :] = 7
    trace = ag._trace
    ag._reserve(2)
    assert ag.trial_steps_trace.shape == (3, 3)
    ag._reserve(5)
    assert ag.trial_steps_trace[:, :3].eq(7).all() and ag.trial_steps_trace[:, 3:].eq(-1).all()
    assert torch.isnan(ag.trial_reward_trace).all() and ag._trace is trace


def test_batched_session_with_trial_end_reports_means():
    env, ag = sequence(3), recording(Stub, 'on_trial_begin', 'on_trial_end')
    ag.train(env, 3)
    kinds = [c[0] for c in ag.calls]
    assert kinds == ['on_trial_begin'] * 3 + ['run', 'after'] + ['on_trial_end'] * 3
    assert of(ag.calls, 'on_trial_begin') == [
        {'trial_reward': 0.0, 'trial': t, 'trial_session': t} for t in range(3)]
    ends = of(ag.calls, 'on_trial_end')
    for t, logs in enumerate(ends):
        assert set(logs) == {'trial_reward', 'trial', 'trial_session', 'steps', 'count'}
        assert logs == {'trial_reward': 10.0 * t + 1.0, 'trial': t, 'trial_session': t,
                        'steps': t + 1.0, 'count': 3}
        assert type(logs['trial_reward']) is float and type(logs['steps']) is float


def test_one_instance_with_trial_end_runs_trial_by_trial_and_honours_stop():
    env, ag = sequence(1), recording(Stub, 'on_trial_end', stop_after=2)
    ag.train(env, 3)
    assert of(ag.calls, 'run') == [(0, 1, STEPS, 0), (1, 1, STEPS, 0)]
    assert [c[0] for c in ag.calls] == ['run', 'after', 'on_trial_end'] * 2
    assert of(ag.calls, 'on_trial_end') == [
        {'trial_reward': 10.0 * t, 'trial': t, 'trial_session': t, 'step': t, 'steps': t, 'at': t}
        for t in range(2)]
    assert ag.current_trial == 2 and ag.stop
    assert env._h_trial.tolist() == [2] and env._h_step.tolist() == [1]
    assert ag.trial_reward_trace.shape == (1, 3) and torch.isnan(ag.trial_reward_trace[0, 2])


def test_one_instance_with_step_end_runs_step_by_step():
    env, ag = sequence(1), recording(Stub, 'on_step_end', 'on_trial_end')
    ag.record_steps = 4
    ag.train(env, 3)
    assert of(ag.calls, 'run') == [(0, 1, STEPS, 1)] * 2 + [(1, 1, STEPS, 1)] + [(2, 1, STEPS, 1)] * 2
    steps = of(ag.calls, 'on_step_end')
    assert [s['step'] for s in steps] == [0, 1, 0, 0, 1] == of(ag.calls, 'step')
    assert [s['launch'] for s in steps] == [0, 1, 2, 3, 4]
    assert [s['trial'] for s in steps] == [0, 0, 1, 2, 2]
    rewards = [0.25 * (k + 1) for k in range(5)]
    assert [s['trial_reward'] for s in steps] == [
        rewards[0], rewards[0] + rewards[1], rewards[2], rewards[3], rewards[3] + rewards[4]]
    ends = of(ag.calls, 'on_trial_end')
    assert [e['steps'] for e in ends] == [1, 0, 1] and [e['step'] for e in ends] == [1, 0, 1]
    assert [e['trial_reward'] for e in ends] == [rewards[0] + rewards[1], rewards[2],
                                                 rewards[3] + rewards[4]]
    assert all('count' not in e and 'at' not in e for e in ends)
    assert ag.current_trial == 3 and env._h_trial.tolist() == [2] and env._h_step.tolist() == [2]
    # the kernel wrote to the one-row buffer: the host kept the first four rows and stopped there
    assert ag._trace_len.tolist() == [4] and ag._trace.shape == (1, 4, 4)
    assert ag.recorded_steps().tolist() == ag.rows[:4]


def test_without_a_one_trial_launch_any_callback_means_step_by_step():
    env, ag = sequence(1), recording(StepOnlyStub, 'on_trial_end')
    ag.record_steps = 4
    ag.train(env, 3)
    assert of(ag.calls, 'run') == [(0, 1, STEPS, 1)] * 2 + [(1, 1, STEPS, 1)] + [(2, 1, STEPS, 1)] * 2
    ends = of(ag.calls, 'on_trial_end')
    assert [e['steps'] for e in ends] == [1, 0, 1] and all(e['step'] == e['steps'] for e in ends)
    assert [c[0] for c in ag.calls][-2:] == ['after', 'on_trial_end']
    assert ag._step_row is None and ag._trace_len.tolist() == [0]     # that trace is the kernel's
    # more than one instance: batched, as for every agent
    env3, ag3 = sequence(3), recording(StepOnlyStub, 'on_trial_end')
    ag3.train(env3, 3)
    assert of(ag3.calls, 'run') == [(0, 3, STEPS, 0)]


def test_session_half_of_a_launch_struct():
    """``_fill_session`` writes the fields a struct declares and chooses where the steps go."""
    env, ag = sequence(1), Stub()
    ag.record_steps = 6
    ag.train(env, 2)
    run = _lib.RWRun()
    ag._step_len[0] = 1
    ag._fill_session(run, 1, 2, 5, 1)
    assert (run.mid, run.trew, run.steps_done) == tuple(
        t.data_ptr() for t in (ag._mid, ag._trew, ag._steps_done))
    assert (run.trial_reward, run.trial_steps, run.trial_action) == (
        ag.trial_reward_trace.data_ptr(), ag.trial_steps_trace.data_ptr(), None)
    assert (run.trial_cap, run.trial_first, run.trials, run.steps_per_trial, run.step_budget) == \
        (2, 1, 2, 5, 1)
    assert (run.trace, run.trace_len, run.trace_cap) == (
        ag._step_row.data_ptr(), ag._step_len.data_ptr(), 1) and ag._step_len.tolist() == [0]
    for run in (_lib.ANetRun(), _lib.ADQNStep()):      # (the latter has no budget, no action trace)
        ag._fill_session(run, 0, 2, 5, 0)
        assert (run.trace, run.trace_len, run.trace_cap) == (
            ag._trace.data_ptr(), ag._trace_len.data_ptr(), 6)
        assert (run.mid, run.trial_steps, run.trial_cap, run.trials) == (
            ag._mid.data_ptr(), ag.trial_steps_trace.data_ptr(), 2, 2)
    assert not hasattr(run, 'step_budget') and not hasattr(run, 'trial_action')


def test_session_steps_and_plan_session_walk_alike():
    st = rc._step
    short = [[st('A', 1.0)] * n for n in (1, 2, 1, 4, 2)]
    long = [[st('B', 0.0)] * n for n in (3, 1, 5, 2, 2)]
    env = HostSequence([short, long], OBS, Box(0.0, 1.0, (2,)), device='cpu', seed=1, n_envs=3,
                       schedule_of=[1, 0, 1])
    env.commit_session(2, 3)        # into the middle of both schedules
    assert env._h_trial.tolist() == [2, 2, 2]
    lengths = [[len(t) for t in s] for s in (short, long)]

    def brute(i, trials, cap):
        p, total = int(env._h_trial[i]), 0
        for _ in range(trials):
            step = 0
            while True:
                step, total = step + 1, total + 1
                if step >= lengths[env.schedule_of[i]][p]:
                    p += 1
                    break
                if step >= cap:
                    break
        return p, total

    for trials, cap in ((0, 3), (1, 1), (2, 3), (3, 4), (3, 5), (3, 9), (6, 2)):
        want = [brute(i, trials, cap) for i in range(3)]
        assert env.session_steps(trials, cap).tolist() == [w[1] for w in want], (trials, cap)
        assert env.plan_session(trials, cap)[0].tolist() == [w[0] for w in want], (trials, cap)
    assert env.session_steps(3, 5).tolist() == [5 + 2 + 2, 1 + 4 + 2, 5 + 2 + 2]
    for call in (env.plan_session, env.session_steps):
        with pytest.raises(IndexError, match='past the last of the 5 trials'):
            call(4, 5)
    # the accessor the agents read the position through
    assert [int(v) for v in env.step_at(1, 1)] == [3 + 1, 1]
    at, length = env.step_at(slice(None))
    assert at.tolist() == [10 + 4, 3, 10 + 4] and length.tolist() == [5, 1, 5]
