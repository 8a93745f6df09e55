"""Associative network — ``cobel.agent.AssociativeNetwork`` (agent/anet.py:15-374, Donoso et al.
2021) on the kernels of csrc/anet.hip, for a ``Sequence`` environment.

Same constructor, ``train(interface, trials, steps=32)``, ``test``, ``rescale_weights``,
``retrieve_q``, ``update_q``, ``predict_on_batch`` and the attributes ``weights``, ``saturation``,
``learning_rate`` (dicts with the keys ``'excitatory'`` / ``'inhibitory'``), ``noise_amplitude``,
``linear_update``, ``alpha`` (read at every launch), ``d_alpha`` (stored only, as in the reference),
``current_trial`` and ``stop``.  ``weights`` holds the reference's NumPy arrays ``[D, A - 1]`` until
the agent meets its environment and device tensors ``[n_envs, D, A - 1]`` from then on.
``saturation`` and ``learning_rate`` entries are a float, an array ``[D, A - 1]`` or a per-instance
array ``[n_envs, D, A - 1]``.  There are A - 1 outputs: the agent only ever chooses the actions
0 ... A - 2, as the reference's does.

Sessions, launches and callbacks are ``SequenceAgent``'s (agent/agent.py); the logs also carry,
from ``logs.update(experience)``, ``state``, ``action``, ``reward``, ``next_state``, ``terminal``.
Per-trial traces ``trial_reward_trace``, ``trial_steps_trace`` and ``trial_action_trace`` are device
tensors ``[n_envs, trials]``; ``record_steps`` > 0 keeps action, reward, end flag and the A - 1
outputs of that many steps per instance (``recorded_steps``).

Streams: the policy adopts STREAM_POLICY; the noise of ``retrieve_q`` — the reference's
``self.rng.random(A - 1)`` — is A - 1 consecutive draws of STREAM_AGENT.  Seed and instance numbers
are the environment's, so results do not depend on how instances are split.  ``test()`` selects with
``policy`` as the reference's does (agent/anet.py:272); ``policy_test`` is stored only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..interface.gridworld import _as_seed
from ..policy.greedy import EpsilonGreedy
from ..spaces import Box, Discrete
from .agent import SequenceAgent

KEYS = ('excitatory', 'inhibitory')


class AssociativeNetwork(SequenceAgent):
    _who = 'AssociativeNetwork'

    def __init__(self, observation_space, action_space, policy, policy_test=None, saturation=20.0,
                 learning_rate=0.01, noise=1.0, linear_update=False, custom_callbacks=None,
                 rng=None) -> None:
        assert type(observation_space) is Box, 'Wrong observation space!'
        assert type(action_space) is Discrete, 'Wrong action space!'
        super().__init__(observation_space, action_space, custom_callbacks)
        self.dim = int(np.prod(observation_space.shape))
        self.n_actions = int(action_space.n)
        if not 1 <= self.dim <= _lib.RW_MAX_DIM:
            raise NotImplementedError(
                'AssociativeNetwork: observations of %d components — this version serves 1 to %d '
                'components' % (self.dim, _lib.RW_MAX_DIM))
        if not 2 <= self.n_actions <= _lib.ANET_MAX_ACTIONS:
            raise NotImplementedError(
                'AssociativeNetwork: %d actions — this version serves 2 to %d actions'
                % (self.n_actions, _lib.ANET_MAX_ACTIONS))
        if type(policy) is not EpsilonGreedy:
            raise NotImplementedError(
                'AssociativeNetwork: a %s policy — this version serves EpsilonGreedy, selected '
                'inside the kernel' % type(policy).__name__)
        self.policy = policy
        self.policy_test = policy if policy_test is None else policy_test
        self.rng = rng
        shape = (self.dim, self.n_actions - 1)
        self.weights = {k: np.zeros(shape) for k in KEYS}
        self.saturation = saturation if type(saturation) is dict else \
            {k: np.full(shape, saturation) for k in KEYS}
        self.learning_rate = learning_rate if type(learning_rate) is dict else \
            {k: np.full(shape, learning_rate) for k in KEYS}
        self.linear_update = linear_update
        self.noise_amplitude = noise
        self.alpha = 1.0
        self.d_alpha = 0.0
        self._row_width = 2 + self.n_actions      # action, reward, end, q[0] ... q[A - 2]
        self._seed = self._instance_ids = None
        self._instance_base = 0
        self._rows_key, self._rows_dev = {}, {}

    # -- device state -----------------------------------------------------------------------------
    def _bind_to(self, n_envs: int, device) -> None:
        device = torch.device(device)
        N, D, NA = int(n_envs), self.dim, self.n_actions - 1
        if self.n_envs is not None:
            if (self.n_envs, self.device) == (N, device):
                return
            assert self._sessions == 0 and self.n_envs == 1, \
                'an agent stays bound to the instance count / device it first trained on'
            # (bound by an early predict_on_batch, retrieve_q or update_q)
            self.weights = {k: self.weights[k][0].cpu().numpy() for k in KEYS}
            drawn = int(self._agent_ctr[0].item())
        else:
            drawn = 0
        self.n_envs, self.device = N, device
        for k in KEYS:
            w = np.asarray(self.weights[k], dtype=np.float64)
            assert w.size in (D * NA, N * D * NA), \
                'weights[%r] has %d entries, not %d x %d (or %d of them)' % (k, w.size, D, NA, N)
            rows = np.broadcast_to(w.reshape(-1, D, NA), (N, D, NA))
            self.weights[k] = torch.as_tensor(np.array(rows, dtype=np.float64, order='C'),
                                              device=device)
        self.device = self.weights[KEYS[0]].device      # (with its index: 'cuda' is 'cuda:0')
        self._agent_ctr = torch.full((N,), drawn, dtype=torch.int32, device=device)
        self._session_buffers()
        self._rows_key, self._rows_dev = {}, {}

    def _bind_alone(self) -> None:
        """A direct call before the agent has met an environment: one instance, number 0, the seed
        from ``rng``."""
        if self.n_envs is None:
            self._bind_to(1, torch.device('cuda', torch.cuda.current_device()))
        if self._seed is None:
            self._seed = _as_seed(self.rng)

    # -- parameters -------------------------------------------------------------------------------
    def _weights(self, key: str):
        """The device tensor of one matrix (an array assigned since is moved there)."""
        N, D, NA = self.n_envs, self.dim, self.n_actions - 1
        w = self.weights[key]
        if not (torch.is_tensor(w) and w.device == self.device and w.dtype == torch.float64
                and tuple(w.shape) == (N, D, NA) and w.is_contiguous()):
            a = np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float64)
            assert a.size in (D * NA, N * D * NA), 'weights[%r]: [%d, %d] or [%d, %d, %d]' % (
                key, D, NA, N, D, NA)
            a = np.broadcast_to(a.reshape(-1, D, NA), (N, D, NA))
            w = self.weights[key] = torch.as_tensor(np.array(a, order='C'), device=self.device)
        return w

    def _rows(self, name: str, key: str):
        """saturation / learning_rate of one matrix as ``[1 or n_envs, D, A - 1]`` on the device."""
        N, D, NA = self.n_envs, self.dim, self.n_actions - 1
        v = np.asarray(getattr(self, name)[key], dtype=np.float64)
        if v.ndim == 0:
            rows = np.full((1, D, NA), float(v))
        elif v.shape == (D, NA):
            rows = v.reshape(1, D, NA)
        else:
            assert v.shape == (N, D, NA), '%s[%r]: a float, an array [%d, %d] or [%d, %d, %d]' % (
                name, key, D, NA, N, D, NA)
            rows = v
        tag, raw = (name, key), rows.tobytes()
        if self._rows_key.get(tag) != raw:
            self._rows_dev[tag] = torch.as_tensor(np.array(rows, dtype=np.float64, order='C'),
                                                  device=self.device)
            self._rows_key[tag] = raw
        return self._rows_dev[tag]

    def _eps_rows(self, pol):
        eps = np.asarray(pol.epsilon, dtype=np.float64).reshape(-1)
        assert eps.shape[0] in (1, self.n_envs), \
            'epsilon: a float or one entry per environment instance'
        tag, raw = ('epsilon', ''), eps.tobytes()
        if self._rows_key.get(tag) != raw:
            self._rows_dev[tag] = torch.as_tensor(eps.copy(), device=self.device)
            self._rows_key[tag] = raw
        return self._rows_dev[tag]

    def _pair(self, name: str):
        """Both matrices' rows of ``name`` with one row count (the kernel takes one per name)."""
        e, i = (self._rows(name, k) for k in KEYS)
        if e.shape[0] != i.shape[0]:
            e, i = (t.expand(self.n_envs, -1, -1).contiguous() for t in (e, i))
        return e, i

    def _fill(self, run) -> None:
        """What every entry point reads: the matrices, their parameters and the agent's stream."""
        run.We, run.Wi = (_lib.ptr(self._weights(k)) for k in KEYS)
        self._sat, self._lr = self._pair('saturation'), self._pair('learning_rate')
        run.sat_e, run.sat_i = (_lib.ptr(t) for t in self._sat)
        run.lr_e, run.lr_i = (_lib.ptr(t) for t in self._lr)
        run.sat_rows, run.lr_rows = self._sat[0].shape[0], self._lr[0].shape[0]
        run.n, run.n_actions = self.n_envs, self.n_actions
        run.linear_update = int(bool(self.linear_update))
        run.alpha, run.noise = float(self.alpha), float(self.noise_amplitude)
        run.agent_ctr = _lib.ptr(self._agent_ctr)
        run.instance_base, run.instance_ids = self._instance_base, _lib.ptr(self._instance_ids)
        run.seed = self._seed

    # -- traces -----------------------------------------------------------------------------------
    def _trial_traces(self) -> tuple:
        return super()._trial_traces() + ('trial_action_trace',)

    def recorded_steps(self, instance: int = 0) -> np.ndarray:
        """Rows (action, reward, end, q[0] ... q[A - 2]) kept since ``record_steps`` was set."""
        return super().recorded_steps(instance)

    # -- launch -----------------------------------------------------------------------------------
    def _launch(self, interface, pol, learn: bool, first: int, trials: int, steps: int,
                budget: int) -> None:
        run = _lib.ANetRun()
        self._fill(run)
        run.flags = _lib.F_LEARN if learn else 0
        run.eps = _lib.ptr(self._eps_rows(pol))
        run.eps_rows = self._rows_dev[('epsilon', '')].shape[0]
        run.pol_ctr, run.pol_stream = _lib.ptr(pol.counter), pol.stream
        self._fill_session(run, first, trials, steps, budget)
        _lib.check(_lib.lib().cobel_anet_run(C.byref(interface.seq), C.byref(run),
                                             _lib.current_stream(self.device)))

    @staticmethod
    def _experience(interface, step: int, action: int) -> dict:
        """The experience of step ``step`` of the trial instance 0 stands in (agent/anet.py:218-224),
        from the host's tables: the position depends on the schedule alone."""
        t = interface.tables
        at, length = (int(v) for v in interface.step_at(0, step))
        end = step + 1 >= length
        if t['step_scalar'][at]:
            reward = float(t['step_reward'][at, 0])
        else:
            forced = int(t['step_action'][at])
            reward = float(t['step_reward'][at, forced if interface.overwrite and forced >= 0
                                            else action])
        nxt = 0 if end else t['step_obs'][at + 1]      # (row 0 is the zero observation)
        return {'state': t['obs_table'][t['step_obs'][at]].copy(), 'action': action,
                'reward': reward, 'next_state': t['obs_table'][nxt].copy(), 'terminal': 1 - end}

    def _refuse(self, interface) -> None:
        A = int(interface.action_space.n)
        if interface.has_array_rewards and not interface.overwrite and self.n_actions - 1 > A:
            raise IndexError('index %d is out of bounds for axis 0 with size %d: the agent chooses '
                             'among %d actions, the array rewards of the Sequence have %d entries'
                             % (A, A, self.n_actions - 1, A))

    def _open(self, interface, trials: int, steps: int, learn: bool) -> None:
        assert self._seed in (None, interface.seed) or self._sessions == 0, \
            'all streams of an instance derive from the environment seed'
        self._seed, self._instance_base = interface.seed, interface.instance_base
        self._instance_ids = interface.instance_ids

    def _step_logs(self, interface, step: int) -> tuple:
        row = self._step_row[0, 0].cpu().numpy()
        experience = self._experience(interface, step, int(row[0]))
        return experience, experience['reward'], row[2]

    def _trial_logs(self, interface, at: int, last_step: int) -> dict:
        return self._experience(interface, last_step, int(self.trial_action_trace[0, at].item()))

    # -- reference surface ------------------------------------------------------------------------
    def train(self, interface, trials: int, steps: int = 32) -> None:
        self._session(interface, trials, steps, True)

    def test(self, interface, trials: int, steps: int = 32) -> None:
        self._session(interface, trials, steps, False)

    def rescale_weights(self, factor: dict) -> None:
        """agent/anet.py:298-309."""
        self.weights['excitatory'] *= factor['excitatory']
        self.weights['inhibitory'] *= factor['inhibitory']

    def predict_on_batch(self, batch):
        """agent/anet.py:358-374, ``retrieve_q`` row by row — every row takes A - 1 draws of the
        agent's stream: ``[B, A - 1]`` for one instance, the device tensor ``[n_envs, B, A - 1]``
        when vectorised (the same batch for every instance)."""
        self._bind_alone()
        b = torch.as_tensor(batch if torch.is_tensor(batch) else np.ascontiguousarray(batch),
                            device=self.device).to(torch.float64).reshape(-1, self.dim).contiguous()
        out = torch.zeros((self.n_envs, b.shape[0], self.n_actions - 1), dtype=torch.float64,
                          device=self.device)
        run = _lib.ANetRun()
        self._fill(run)
        _lib.check(_lib.lib().cobel_anet_predict(C.byref(run), self.dim, _lib.ptr(b), b.shape[0],
                                                 _lib.ptr(out), _lib.current_stream(self.device)))
        return out[0].cpu().numpy() if self.n_envs == 1 else out

    def retrieve_q(self, observation):
        """agent/anet.py:311-333: ``[A - 1]`` for one instance, ``[n_envs, A - 1]`` when vectorised."""
        out = self.predict_on_batch(np.asarray(observation.detach().cpu() if torch.is_tensor(observation)
                                               else observation, dtype=np.float64).reshape(1, -1))
        return out[0] if self.n_envs == 1 else out[:, 0]

    def update_q(self, experience: dict) -> None:
        """agent/anet.py:335-356 with ``experience['state']``, ``['action']`` and ``['reward']``: one
        experience, or one per instance (``state [n_envs, D]``, ``action`` and ``reward [n_envs]``)."""
        self._bind_alone()
        N = self.n_envs

        def per_instance(v, dtype, shape):
            a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=dtype)
            a = np.broadcast_to(a.reshape((-1,) + shape), (N,) + shape)
            return torch.as_tensor(np.array(a, order='C'), device=self.device)

        state = per_instance(experience['state'], np.float64, (self.dim,))
        action = per_instance(experience['action'], np.int32, ())
        reward = per_instance(experience['reward'], np.float64, ())
        run = _lib.ANetRun()
        self._fill(run)
        _lib.check(_lib.lib().cobel_anet_update(C.byref(run), self.dim, _lib.ptr(state),
                                                _lib.ptr(action), _lib.ptr(reward),
                                                _lib.current_stream(self.device)))
