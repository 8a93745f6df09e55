"""``QAgent`` on a ``Sequence`` — the part of ``cobel.agent.QAgent`` (agent/q.py:26-354) that a
gridworld's tables cannot serve: Q keyed by the observation itself, float64, with a ``Softmax`` or an
``EpsilonGreedy`` policy, on the kernel of csrc/qseq.hip.

``QSequence`` is the helper a ``QAgent`` hands a ``Sequence`` session to.  It is a ``SequenceAgent``:
sessions, launches and callbacks are that driver's; the callbacks, ``current_trial``, ``stop``, the
policies and the hyper-parameters stay the owner's, so ``logs['agent']`` is the ``QAgent``.

Keys.  The reference keys ``Q`` by ``tuple(observation.flatten())``: observations of equal values
share a row, and the zero observation a trial ends in is a key as well.  The rows of the Sequence's
observation table are deduplicated by value (``observation_keys``); the kernel sees key indices.
The reference creates a row when it first meets a key; which keys an instance meets depends on the
schedule and the step caps alone, so the host walks instance 0's schedule and ``Q_dict`` holds
exactly the keys the reference's dict would, in its order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..policy.greedy import EpsilonGreedy
from ..policy.softmax import Softmax
from ..spaces import Box
from .agent import SequenceAgent


def observation_keys(obs_table: np.ndarray) -> tuple:
    """``(key_of_row [n_obs] int32, key_obs [n_keys, D])``: rows of equal values share a key; keys
    are numbered by first appearance, so the zero observation (row 0) is key 0."""
    table = np.ascontiguousarray(np.asarray(obs_table, dtype=np.float64))
    table = table.reshape(len(table), -1)
    seen: dict = {}
    key_of_row = np.empty(len(table), dtype=np.int32)
    for r, row in enumerate(table):
        key_of_row[r] = seen.setdefault(tuple(row.tolist()), len(seen))
    key_obs = np.array([list(k) for k in seen], dtype=np.float64).reshape(len(seen), table.shape[1])
    return key_of_row, key_obs


class QSequence(SequenceAgent):
    _who = 'QAgent'
    _row_width = _lib.QSEQ_ROW     # state key, action, reward, next key, non-terminal, td

    def __init__(self, owner) -> None:
        self.__dict__['owner'] = owner
        if type(owner.observation_space) is not Box:
            raise NotImplementedError(
                'QAgent on a Sequence: %s observation spaces — this version serves Box observation '
                'spaces' % type(owner.observation_space).__name__)
        trial, stop = owner.current_trial, owner.stop
        super().__init__(owner.observation_space, owner.action_space, None)
        self.current_trial, self.stop = trial, stop
        self.callbacks = owner.callbacks
        self.dim = int(np.prod(owner.observation_space.shape))
        self.n_actions = int(owner.action_space.n)
        if not 1 <= self.n_actions <= _lib.QSEQ_MAX_ACTIONS:
            raise NotImplementedError('QAgent on a Sequence: %d actions — this version serves 1 to %d'
                                      % (self.n_actions, _lib.QSEQ_MAX_ACTIONS))
        self.key_of_row = self.key_obs = None
        self._q = self._log = self._log_len = self._mem_ctr = self._last = self._keys_dev = None
        self._log_cap = 0
        self._par_key = self._par_dev = None
        self._batch = 32
        self.created: list = []       # keys of instance 0's dict, in the order the reference makes them
        self._pending: list = []      # per trial of the open session: the keys it will meet

    # -- what stays the owner's -------------------------------------------------------------------
    current_trial = property(lambda self: self.owner.current_trial,
                             lambda self, v: setattr(self.owner, 'current_trial', v))
    stop = property(lambda self: self.owner.stop, lambda self, v: setattr(self.owner, 'stop', v))
    policy = property(lambda self: self.owner.policy, lambda self, v: None)
    policy_test = property(lambda self: self.owner.policy_test, lambda self, v: None)

    # -- binding ----------------------------------------------------------------------------------
    def _bind_to(self, n_envs: int, device) -> None:
        device = torch.device(device)
        if self.n_envs is not None:
            assert (self.n_envs, self.device) == (int(n_envs), device), \
                'an agent stays bound to the instance count / device it first trained on'
            return
        self.n_envs, self.device = int(n_envs), device
        N, K, A = self.n_envs, len(self.key_obs), self.n_actions
        self._q = torch.zeros((N, K, A), dtype=torch.float64, device=device)
        self._log_len = torch.zeros(N, dtype=torch.int32, device=device)
        self._mem_ctr = torch.zeros(N, dtype=torch.int32, device=device)
        self._last = torch.zeros((N, self._row_width), dtype=torch.float64, device=device)
        self._keys_dev = torch.as_tensor(self.key_of_row, device=device)
        self._session_buffers()

    def _refuse(self, interface) -> None:
        for pol in (self.policy, self.policy_test):
            if not isinstance(pol, (Softmax, EpsilonGreedy)):
                raise NotImplementedError('QAgent on a Sequence takes the Softmax and EpsilonGreedy '
                                          'policies, not %s' % type(pol).__name__)
        assert int(interface.action_space.n) == self.n_actions, \
            'the Sequence has %d actions, the agent %d' % (int(interface.action_space.n),
                                                          self.n_actions)
        key_of_row, key_obs = observation_keys(interface.tables['obs_table'])
        if self.key_obs is None:
            if len(key_obs) > _lib.QSEQ_MAX_KEYS:
                raise NotImplementedError(
                    'QAgent on a Sequence: %d distinct observations — this version serves up to %d'
                    % (len(key_obs), _lib.QSEQ_MAX_KEYS))
            self.key_of_row, self.key_obs = key_of_row, key_obs
        elif not (np.array_equal(key_of_row, self.key_of_row)
                  and np.array_equal(key_obs, self.key_obs)):
            raise NotImplementedError('QAgent on a Sequence stays with the observations of the '
                                      'Sequence it first met')

    def reserve_replay(self, entries: int) -> None:
        """Room for ``entries`` logged experiences per instance (16 B each)."""
        if entries <= self._log_cap:
            return
        new = torch.zeros((self.n_envs, int(entries), 2), dtype=torch.int64, device=self.device)
        if self._log is not None:
            new[:, :self._log_cap] = self._log
        self._log, self._log_cap = new, int(entries)

    # -- policies and parameters ------------------------------------------------------------------
    def _acting_policy(self, learn: bool):
        """agent/q.py:199, :263: ``train`` selects with ``policy``, ``test`` with ``policy_test``."""
        return self.policy if learn else self.policy_test

    def _policy_in(self, pol, interface) -> None:
        # (a distinct policy_test draws from a stream of its own, as with the tabular agents)
        if pol.stream is None and pol is not self.policy:
            pol.stream = _lib.STREAM_POLICY_TEST
        super()._policy_in(pol, interface)

    def _par_rows(self, pol):
        N = self.n_envs
        cols = [np.asarray(self.owner.learning_rate, dtype=np.float64),
                np.asarray(self.owner.gamma, dtype=np.float64),
                np.asarray(pol.beta if isinstance(pol, Softmax) else pol.epsilon, dtype=np.float64)]
        for c in cols:
            assert c.ndim == 0 or c.shape == (N,), \
                'per-instance hyper-parameters need one entry per environment instance'
        rows = 1 if all(c.ndim == 0 for c in cols) else N
        par = np.zeros((rows, 4), dtype=np.float64)
        for k, c in enumerate(cols):
            par[:, k] = c
        key = par.tobytes()
        if key != self._par_key:
            self._par_dev = torch.as_tensor(par, device=self.device)
            self._par_key = key
        return self._par_dev

    # -- the keys the reference's dict holds ------------------------------------------------------
    def _open(self, interface, trials: int, steps: int, learn: bool, batch_size: int = 32) -> None:
        self._batch = int(batch_size)
        if learn:
            used = int(self._log_len.max().item())
            self.reserve_replay(used + int(interface.session_steps(trials, steps).max()))
        # instance 0's walk through its schedule: the state of every step it takes and, in train(),
        # the observation that step leads to (agent/q.py:197-204, :261-262)
        tab, sched = interface.tables, int(interface.schedule_of[0])
        p, self._pending = int(interface._h_trial[0]), []
        for _ in range(trials):
            base, length = int(tab['trial_off'][sched, p]), int(interface._trial_len[sched, p])
            met = []
            for k in range(min(length, steps)):
                met.append(int(self.key_of_row[tab['step_obs'][base + k]]))
                if learn:
                    met.append(int(self.key_of_row[tab['step_obs'][base + k + 1]])
                               if k + 1 < length else int(self.key_of_row[0]))
            self._pending.append(met)
            p += int(length <= steps)

    def _after_trial(self, logs=None):
        done = self._pending if logs is None else self._pending[:1]
        for met in done:
            for k in met:
                if k not in self.created:
                    self.created.append(k)
        del self._pending[:len(done)]
        return logs

    # -- launch -----------------------------------------------------------------------------------
    def _launch(self, interface, pol, learn: bool, first: int, trials: int, steps: int,
                budget: int) -> None:
        if trials == 0:
            return
        run = _lib.QSeqRun()
        ptr = _lib.ptr
        run.Q, run.key_of_row, run.par = ptr(self._q), ptr(self._keys_dev), ptr(self._par_rows(pol))
        run.par_rows = self._par_dev.shape[0]
        run.pol_ctr, run.pol_stream = ptr(pol.counter), pol.stream
        run.mem_ctr, run.log, run.log_len = ptr(self._mem_ctr), ptr(self._log), ptr(self._log_len)
        if self._log is None:
            run.log_len = None
        run.log_cap = self._log_cap
        run.last = ptr(self._last)
        run.n, run.n_keys, run.n_actions = self.n_envs, len(self.key_obs), self.n_actions
        run.policy = _lib.QSEQ_POLICY_SOFTMAX if isinstance(pol, Softmax) \
            else _lib.QSEQ_POLICY_EPS_GREEDY
        run.batch_size = self._batch if learn else 0
        run.flags = _lib.F_LEARN if learn else 0
        run.instance_base, run.instance_ids = interface.instance_base, ptr(interface.instance_ids)
        run.seed = interface.seed
        self._fill_session(run, first, trials, steps, budget)
        _lib.check(_lib.lib().cobel_qseq_run(C.byref(interface.seq), C.byref(run),
                                             _lib.current_stream(self.device)))

    def _entries(self, row: np.ndarray, learn: bool) -> dict:
        out = {'state': self.key_tuple(int(row[0])), 'action': int(row[1]), 'reward': float(row[2]),
               'next_state': self.key_tuple(int(row[3])), 'terminal': int(row[4])}
        if learn:
            out['td'] = float(row[5])
        return out

    def _step_logs(self, interface, step: int) -> tuple:
        row = self._step_row[0, 0].cpu().numpy()
        return self._entries(row, self._learning), float(row[2]), row[4] == 0

    def _trial_logs(self, interface, at: int, last_step: int) -> dict:
        return self._entries(self._last[0].cpu().numpy(), self._learning)

    def train(self, interface, trials: int, steps: int = 32, batch_size: int = 32) -> None:
        assert batch_size >= 0
        self._learning = True
        self._session(interface, trials, steps, True, batch_size=batch_size)

    def test(self, interface, trials: int, steps: int = 32) -> None:
        self._learning = False
        self._session(interface, trials, steps, False, batch_size=0)

    # -- the reference's views --------------------------------------------------------------------
    def key_tuple(self, key: int) -> tuple:
        return tuple(self.key_obs[key].tolist())

    @property
    def Q_dict(self) -> dict:
        if self._q is None:
            return {}
        q = self._q[0].cpu().numpy()
        return {self.key_tuple(k): q[k] for k in self.created}

    @property
    def M(self) -> list:
        if self._log is None:
            return []
        n = int(self._log_len[0].item())
        raw = self._log[0, :n].cpu().numpy()
        rew, meta = raw[:, 0].copy().view(np.float64), raw[:, 1]
        return [{'state': self.key_tuple(int(m & 0xFF)), 'action': int((m >> 16) & 0xFF),
                 'reward': float(r), 'next_state': self.key_tuple(int((m >> 8) & 0xFF)),
                 'terminal': int((m >> 24) & 1)} for r, m in zip(rew, meta)]

    def predict_on_batch(self, batch):
        """agent/q.py:333-334: a ``KeyError`` for an observation the agent has not met."""
        obs = np.asarray(batch, dtype=np.float64).reshape(len(batch), -1)
        keys = []
        for o in obs:
            hit = [k for k in self.created if np.array_equal(self.key_obs[k], o)]
            if not hit:
                raise KeyError(tuple(o.tolist()))
            keys.append(hit[0])
        if self.n_envs == 1:
            return self._q[0].cpu().numpy()[keys]
        return self._q[:, torch.as_tensor(keys, device=self.device)]
