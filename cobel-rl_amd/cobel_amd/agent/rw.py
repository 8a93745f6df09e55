"""Rescorla-Wagner agents — ``cobel.agent.RescorlaWagner`` and ``BinaryRescorlaWagner``
(agent/rw.py:15-376) on the kernels of csrc/rw.hip, for a ``Sequence`` environment.

Same constructors, ``train(interface, trials, steps=32)``, ``test``, ``predict_on_batch`` and the
attributes ``W``, ``learning_rate``, ``current_trial``, ``stop`` (and ``policy`` / ``policy_test``).
``W`` is the reference's NumPy array until the agent meets its environment and the device tensor
``[n_envs, D]`` from then on; both take ``W.fill(0.5)`` and assignment.  ``learning_rate`` is a
float, a tuple of length D as in the reference, or an array ``[n_envs]`` or ``[n_envs, D]`` (an
array of length D is the reference's tuple, also where ``n_envs == D``).

The classes derive from ``Agent``, not from ``FusedAgent``: that one's device state is built around
a world handle (states, action masks, start draws), of which a Sequence has none.  The launch
convention is the same: one launch per session for ``n_envs > 1``; for ``n_envs == 1`` with
callbacks one per trial, or per step where step callbacks are registered, with the reference's log
keys (``trial_reward``, ``trial``, ``trial_session``, ``step``, ``steps`` and, for the binary agent,
``action``).  Per-trial traces ``trial_reward_trace``, ``trial_steps_trace`` and (binary)
``trial_action_trace`` are device tensors ``[n_envs, trials]``; ``record_steps`` > 0 keeps value,
action, reward and end flag of that many steps per instance (``recorded_steps``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..policy.scalar import ScalarPolicy
from ..spaces import Box, Discrete
from .agent import Agent


class Weights(torch.Tensor):
    """The device tensor of the weights under NumPy's method name: ``agent.W.fill(0.5)``."""

    def fill(self, value) -> None:
        self.fill_(value)


class RescorlaWagner(Agent):
    _who = 'RescorlaWagner'

    def __init__(self, observation_space, learning_rate=0.9, custom_callbacks=None) -> None:
        assert type(observation_space) is Box, 'Wrong observation space!'
        super().__init__(observation_space, Box(-np.inf, np.inf, (1,), np.float64), custom_callbacks)
        self.dim = int(np.prod(observation_space.shape))
        if not 1 <= self.dim <= _lib.RW_MAX_DIM:
            raise NotImplementedError(
                '%s: observations of %d components — this version serves 1 to %d components'
                % (self._who, self.dim, _lib.RW_MAX_DIM))
        self._W = np.zeros(observation_space.shape)
        if type(learning_rate) is float:
            self.learning_rate = learning_rate
        else:
            self.learning_rate = np.array(learning_rate)
        self.policy = self.policy_test = None
        self.record_steps = 0         # > 0: keep that many steps' (value, action, reward, end)
        self.n_envs = self.device = None
        self.trial_reward_trace = self.trial_steps_trace = self.trial_action_trace = None
        self._trace = self._trace_len = None
        self._sessions = 0
        self._lr_key = self._lr_dev = None
        self._pol_key = self._pol_dev = None

    # -- the weights ------------------------------------------------------------------------------
    @property
    def W(self):
        return self._W

    @W.setter
    def W(self, value) -> None:
        if self.n_envs is None:
            self._W = np.array(value, dtype=np.float64)
            return
        v = torch.as_tensor(np.asarray(value.detach().cpu() if torch.is_tensor(value) else value,
                                       dtype=np.float64), device=self.device)
        self._W.copy_(v.reshape(-1, self.dim) if v.numel() != self.dim else v.reshape(1, self.dim))

    def _bind_to(self, n_envs: int, device) -> None:
        device = torch.device(device)
        if self.n_envs is not None:
            if (self.n_envs, self.device) == (int(n_envs), device):
                return
            assert self._sessions == 0 and self.n_envs == 1, \
                'an agent stays bound to the instance count / device it first trained on'
            self._W = self._W[0].cpu().numpy()      # (bound by an early predict_on_batch)
        N, D = int(n_envs), self.dim
        w = np.asarray(self._W, dtype=np.float64)
        assert w.size in (D, N * D), 'W has %d entries, not %d (or %d x %d)' % (w.size, D, N, D)
        rows = np.broadcast_to(w.reshape(-1, D), (N, D))
        self.n_envs, self.device = N, device
        self._W = torch.as_tensor(np.array(rows, dtype=np.float64, order='C'), device=device).as_subclass(Weights)
        self._mid = torch.zeros(N, dtype=torch.int32, device=device)
        self._trew = torch.zeros(N, dtype=torch.float64, device=device)
        self._steps_done = torch.zeros(1, dtype=torch.int64, device=device)
        self._step_row = torch.zeros((N, 1, 4), dtype=torch.float64, device=device)
        self._step_len = torch.zeros(N, dtype=torch.int32, device=device)
        self._lr_key = self._pol_key = None

    def env_steps(self) -> int:
        return int(self._steps_done.item()) if self.n_envs is not None else 0

    # -- parameters -------------------------------------------------------------------------------
    def _lr_rows(self):
        N, D = self.n_envs, self.dim
        lr = np.asarray(self.learning_rate, dtype=np.float64)
        if lr.ndim == 0:
            rows = np.full((1, D), float(lr))
        elif lr.shape == (D,):
            rows = lr.reshape(1, D)
        elif lr.shape == (N,):
            rows = np.broadcast_to(lr.reshape(N, 1), (N, D))
        else:
            assert lr.shape == (N, D), \
                'learning_rate: a float, %d values, or an array [%d] or [%d, %d]' % (D, N, N, D)
            rows = lr
        key = rows.tobytes()
        if key != self._lr_key:
            self._lr_dev = torch.as_tensor(np.array(rows, dtype=np.float64, order='C'),
                                           device=self.device)
            self._lr_key = key
        return self._lr_dev

    def _pol_rows(self, pol):
        rows = pol.parameter_rows(self.n_envs)
        key = (id(pol), rows.tobytes())
        if key != self._pol_key:
            self._pol_dev = torch.as_tensor(rows, device=self.device)
            self._pol_key = key
        return self._pol_dev

    def _refuse(self, interface) -> None:
        if interface.has_array_rewards and not interface.overwrite:
            raise NotImplementedError(
                'RescorlaWagner: the Sequence has array rewards and overwrite=False — the reference '
                'would index the reward with int(value) (interface/sequence.py:165); this version '
                'serves array rewards with overwrite=True only')

    # -- traces -----------------------------------------------------------------------------------
    def _reserve(self, trials: int) -> None:
        names = ['trial_reward_trace', 'trial_steps_trace']
        if self.policy is not None:
            names.append('trial_action_trace')
        for name in names:
            old = getattr(self, name)
            if old is not None and old.shape[1] >= trials:
                continue
            if name == 'trial_reward_trace':
                new = torch.full((self.n_envs, trials), float('nan'), dtype=torch.float64,
                                 device=self.device)
            else:
                new = torch.full((self.n_envs, trials), -1, dtype=torch.int32, device=self.device)
            if old is not None:
                new[:, :old.shape[1]] = old
            setattr(self, name, new)
        if self.record_steps and self._trace is None:
            self._trace = torch.zeros((self.n_envs, int(self.record_steps), 4), dtype=torch.float64,
                                      device=self.device)
            self._trace_len = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)

    def recorded_steps(self, instance: int = 0) -> np.ndarray:
        """Rows (value, action, reward, end) kept since ``record_steps`` was set."""
        n = int(self._trace_len[instance].item())
        return self._trace[instance, :n].cpu().numpy()

    # -- launch -----------------------------------------------------------------------------------
    def _launch(self, interface, pol, learn: bool, first: int, trials: int, steps: int,
                budget: int) -> None:
        run = _lib.RWRun()
        run.W, run.lr = _lib.ptr(self._W), _lib.ptr(self._lr_rows())
        run.lr_rows = self._lr_dev.shape[0]
        run.n, run.flags = self.n_envs, _lib.F_LEARN if learn else 0
        run.instance_base, run.instance_ids = interface.instance_base, _lib.ptr(interface.instance_ids)
        run.seed = interface.seed
        run.mid, run.trew, run.steps_done = _lib.ptr(self._mid), _lib.ptr(self._trew), \
            _lib.ptr(self._steps_done)
        run.trial_reward, run.trial_steps = _lib.ptr(self.trial_reward_trace), \
            _lib.ptr(self.trial_steps_trace)
        run.trial_action = _lib.ptr(self.trial_action_trace)
        run.trial_cap = self.trial_reward_trace.shape[1]
        if budget == 1:         # a launch per step: the step comes back in a row of its own
            self._step_len.zero_()
            run.trace, run.trace_len, run.trace_cap = _lib.ptr(self._step_row), \
                _lib.ptr(self._step_len), 1
        elif self._trace is not None:
            run.trace, run.trace_len = _lib.ptr(self._trace), _lib.ptr(self._trace_len)
            run.trace_cap = self._trace.shape[1]
        run.policy = _lib.RW_POLICY_NONE
        if pol is not None:
            run.policy, run.code_reverse = pol.kind, int(bool(pol.code_reverse))
            run.pol = _lib.ptr(self._pol_rows(pol))
            run.pol_rows = self._pol_dev.shape[0]
            run.pol_ctr, run.pol_stream = _lib.ptr(pol.counter), pol.stream
        run.trial_first, run.trials, run.steps_per_trial, run.step_budget = first, trials, steps, budget
        _lib.check(_lib.lib().cobel_rw_run(C.byref(interface.seq), C.byref(run),
                                           _lib.current_stream(self.device)))

    def _policy_in(self, pol, interface) -> None:
        """Adopt the policy's stream and draw counters.  It is always ``policy`` and its stream
        STREAM_POLICY: the reference selects with ``policy`` in ``test()`` too (agent/rw.py:359);
        ``policy_test`` is stored only."""
        if pol.seed is None:
            pol.seed = interface.seed
        assert pol.seed == interface.seed, 'all streams of an instance derive from the environment seed'
        if pol.stream is None:
            pol.stream = _lib.STREAM_POLICY
        if pol.counter is None or pol.counter.numel() != self.n_envs or \
                pol.counter.device != self.device:
            pol.counter = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)

    def _session(self, interface, trials: int, steps: int, learn: bool) -> None:
        if not hasattr(interface, 'seq'):
            raise NotImplementedError('%s runs on a Sequence' % self._who)
        assert interface.dim == self.dim, \
            'the Sequence has observations of %d components, the agent %d' % (interface.dim, self.dim)
        self._refuse(interface)
        trials, steps = int(trials), int(steps)
        assert steps >= 1, 'steps must be at least 1'
        interface.plan_session(trials, steps)      # IndexError here, before any launch
        interface._on_device()
        self._bind_to(interface.n_envs, interface.device)
        # (the reference's BinaryRescorlaWagner.test selects with `policy`, not `policy_test`:
        #  agent/rw.py:359 — kept; `policy_test` is stored as there)
        pol = self.policy
        if pol is not None:
            self._policy_in(pol, interface)
        first = self.current_trial
        self._reserve(first + trials)
        self._sessions += 1
        binary = pol is not None
        per_step = self.n_envs == 1 and self.callbacks.has('on_step_begin', 'on_step_end')
        per_trial = self.n_envs == 1 and (per_step or self.callbacks.has('on_trial_begin',
                                                                         'on_trial_end'))
        if not per_trial:
            for t in range(trials):
                self.callbacks.on_trial_begin({'trial_reward': 0.0, 'trial': first + t,
                                               'trial_session': t})
            self._launch(interface, pol, learn, first, trials, steps, 0)
            interface.commit_session(trials, steps)
            self.current_trial = first + trials
            if self.callbacks.has('on_trial_end'):
                rew = self.trial_reward_trace[:, first:first + trials].mean(dim=0).cpu().numpy()
                lat = self.trial_steps_trace[:, first:first + trials].double().mean(dim=0).cpu().numpy()
                for t in range(trials):
                    self.callbacks.on_trial_end({
                        'trial_reward': float(rew[t]), 'trial': first + t, 'trial_session': t,
                        'steps': float(lat[t]), 'count': self.n_envs})
            return
        for t in range(trials):
            logs = self.callbacks.on_trial_begin({'trial_reward': 0.0, 'trial': self.current_trial,
                                                  'trial_session': t})
            at = self.current_trial
            if per_step:
                step = 0
                while True:
                    logs['step'] = step
                    logs = self.callbacks.on_step_begin(logs)
                    self._launch(interface, pol, learn, at, 1, steps, 1)
                    value, action, reward, end = self._step_row[0, 0].cpu().numpy()
                    if self._trace is not None:
                        n = int(self._trace_len[0].item())
                        if n < self._trace.shape[1]:
                            self._trace[0, n] = self._step_row[0, 0]
                            self._trace_len[0] = n + 1
                    logs['trial_reward'] += float(reward)
                    if binary:
                        logs['action'] = int(action)
                    logs = self.callbacks.on_step_end(logs)
                    step += 1
                    if end or step >= steps:
                        break
                logs['steps'] = step - 1
            else:
                self._launch(interface, pol, learn, at, 1, steps, 0)
                logs['step'] = logs['steps'] = int(self.trial_steps_trace[0, at].item())
                logs['trial_reward'] = float(self.trial_reward_trace[0, at].item())
                if binary:
                    logs['action'] = int(self.trial_action_trace[0, at].item())
            interface.commit_session(1, steps)
            self.current_trial += 1
            logs = self.callbacks.on_trial_end(logs)
            if self.stop:
                break

    # -- reference surface ------------------------------------------------------------------------
    def train(self, interface, trials: int, steps: int = 32) -> None:
        self._session(interface, trials, steps, True)

    def test(self, interface, trials: int, steps: int = 32) -> None:
        self._session(interface, trials, steps, False)

    def predict_on_batch(self, batch):
        """agent/rw.py:176-192, ``W @ batch.T``: ``[B]`` for one instance, the device tensor
        ``[n_envs, B]`` when vectorised."""
        assert type(batch) is np.ndarray or torch.is_tensor(batch)
        if self.n_envs is None:
            self._bind_to(1, torch.device('cuda', torch.cuda.current_device()))
        b = torch.as_tensor(batch, device=self.device).to(torch.float64).reshape(-1, self.dim).contiguous()
        out = torch.zeros((self.n_envs, b.shape[0]), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().cobel_rw_predict(_lib.ptr(self._W), self.n_envs, self.dim, _lib.ptr(b),
                                               b.shape[0], _lib.ptr(out),
                                               _lib.current_stream(self.device)))
        return out[0].cpu().numpy() if self.n_envs == 1 else out


class BinaryRescorlaWagner(RescorlaWagner):
    _who = 'BinaryRescorlaWagner'

    def __init__(self, observation_space, policy, policy_test=None, learning_rate=0.9,
                 custom_callbacks=None) -> None:
        assert type(observation_space) is Box, 'Wrong observation space!'
        super().__init__(observation_space, learning_rate, custom_callbacks)
        assert isinstance(policy, ScalarPolicy) and \
            (policy_test is None or isinstance(policy_test, ScalarPolicy)), \
            'BinaryRescorlaWagner takes the scalar policies Proportional, Threshold and Sigmoid'
        self.action_space = Discrete(2)
        self.policy = policy
        self.policy_test = policy if policy_test is None else policy_test

    def _refuse(self, interface) -> None:
        if interface.has_array_rewards:
            raise NotImplementedError(
                'BinaryRescorlaWagner: the Sequence has array rewards — the reference asserts '
                'type(reward) is float (agent/rw.py:302); this version serves float rewards')
