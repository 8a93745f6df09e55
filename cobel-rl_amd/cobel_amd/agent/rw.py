"""Rescorla-Wagner agents — ``cobel.agent.RescorlaWagner`` and ``BinaryRescorlaWagner``
(agent/rw.py:15-376) on the kernels of csrc/rw.hip, for a ``Sequence`` environment.

Same constructors, ``train(interface, trials, steps=32)``, ``test``, ``predict_on_batch`` and the
attributes ``W``, ``learning_rate``, ``current_trial``, ``stop`` (and ``policy`` / ``policy_test``).
``W`` is the reference's NumPy array until the agent meets its environment and the device tensor
``[n_envs, D]`` from then on; both take ``W.fill(0.5)`` and assignment.  ``learning_rate`` is a
float, a tuple of length D as in the reference, or an array ``[n_envs]`` or ``[n_envs, D]`` (an
array of length D is the reference's tuple, also where ``n_envs == D``).

Sessions, launches and callbacks are ``SequenceAgent``'s (agent/agent.py); the binary agent adds
``action`` to the logs.  Per-trial traces ``trial_reward_trace``, ``trial_steps_trace`` and (binary)
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
from .agent import SequenceAgent


class Weights(torch.Tensor):
    """The device tensor of the weights under NumPy's method name: ``agent.W.fill(0.5)``."""

    def fill(self, value) -> None:
        self.fill_(value)


class RescorlaWagner(SequenceAgent):
    _who = 'RescorlaWagner'
    _row_width = 4      # value, action, reward, end

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
        self._session_buffers()
        self._lr_key = self._pol_key = None

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
    def _trial_traces(self) -> tuple:
        names = super()._trial_traces()
        return names if self.policy is None else names + ('trial_action_trace',)

    def recorded_steps(self, instance: int = 0) -> np.ndarray:
        """Rows (value, action, reward, end) kept since ``record_steps`` was set."""
        return super().recorded_steps(instance)

    # -- launch -----------------------------------------------------------------------------------
    def _launch(self, interface, pol, learn: bool, first: int, trials: int, steps: int,
                budget: int) -> None:
        run = _lib.RWRun()
        run.W, run.lr = _lib.ptr(self._W), _lib.ptr(self._lr_rows())
        run.lr_rows = self._lr_dev.shape[0]
        run.n, run.flags = self.n_envs, _lib.F_LEARN if learn else 0
        run.instance_base, run.instance_ids = interface.instance_base, _lib.ptr(interface.instance_ids)
        run.seed = interface.seed
        self._fill_session(run, first, trials, steps, budget)
        run.policy = _lib.RW_POLICY_NONE
        if pol is not None:
            run.policy, run.code_reverse = pol.kind, int(bool(pol.code_reverse))
            run.pol = _lib.ptr(self._pol_rows(pol))
            run.pol_rows = self._pol_dev.shape[0]
            run.pol_ctr, run.pol_stream = _lib.ptr(pol.counter), pol.stream
        _lib.check(_lib.lib().cobel_rw_run(C.byref(interface.seq), C.byref(run),
                                           _lib.current_stream(self.device)))

    def _step_logs(self, interface, step: int) -> tuple:
        value, action, reward, end = self._step_row[0, 0].cpu().numpy()
        return ({} if self.policy is None else {'action': int(action)}), float(reward), end

    def _trial_logs(self, interface, at: int, last_step: int) -> dict:
        if self.policy is None:
            return {}
        return {'action': int(self.trial_action_trace[0, at].item())}

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
