"""PMA agent — ``cobel.agent.PMA`` (agent/pma.py:16-369): Dyna-Q with Prioritized Memory Access
(Mattar & Daw 2018) on the kernels of csrc/pma.hip.

Same constructor, ``train(interface, trials, steps, batch_size=32, no_replay=False)``, ``test``,
``update_q``, ``predict_on_batch`` and attributes (``Q``, ``M``, ``learning_rate``, ``gamma``,
``action_mask``, ``mask_actions``), plus the ``on_replay_end`` callback with ``logs['replay']``.
``Q`` is float64, as the reference's.  Worlds of more than 128 states take a memory built with
``PMAMemory(..., wide=True)``; the agent follows ``memory.wide``.  As in the reference, ``test()`` draws its actions from
``policy`` (``policy_test`` is stored and not consulted, agent/pma.py:291).

``train`` runs trial by trial over all instances: ``cobel_pma_trial`` (reset, the start-of-trial
replay, the steps with the 1-step update and the store), then ``M.update_sr()`` through the public
method, then the end-of-trial replay with need from ``SR[last]``.  Instances whose trial timed out
have no last state: their need is ``M.compute_need(None)``.  With ``M.offline_need == 'host'`` (the
default) that runs on the host, so ``last`` [N] is read back once per trial and T with it where a
trial timed out.  With ``M.offline_need = 'device'`` the trial is four device calls —
``cobel_pma_trial``, ``update_sr``, ``cobel_pma_stationary`` selecting by ``last``, ``cobel_pma_replay``
with ``last`` and that need tensor — and nothing is read back unless a callback asks for host
values.  A wide memory built with a ``need_workspace`` takes ``cobel_pma_stationary_wide`` in that
place (the elimination on a workspace in device memory), with the same effect.  Host callbacks fire at these boundaries: ``on_replay_end`` of the start
replay after the trial's kernel, step callbacks not at all.  The head and the tail of a session
are ``FusedAgent._session_begin`` / ``_session_end``; the loop between them is this agent's.

``learning_rate``, ``gamma`` and the acting policy's ``epsilon`` take a scalar or one entry per
instance, as the memory's parameters do (memory/pma.py): a sweep rides on the instance axis, the
trial stays four device calls.  The memory's ``_fill_params`` builds the parameter sets for the
launcher and for ``update_q``; ``batch_size`` is launch-wide.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..spaces import Discrete
from ..memory import _device
from ..memory.pma import launch_wide
from .agent import Callbacks, FusedAgent


class CallbacksPMA(Callbacks):
    def on_replay_end(self, logs: dict) -> dict:
        return self._fire('on_replay_end', logs)


class PMA(FusedAgent):
    CallbacksPMA = CallbacksPMA
    general_actions = True

    def __init__(self, observation_space, action_space, policy, memory, policy_test=None,
                 learning_rate: float = 0.9, gamma: float = 0.99, custom_callbacks=None) -> None:
        assert type(observation_space) is Discrete, 'PMA requires a discrete observation space!'
        assert type(action_space) is Discrete, 'PMA requires a discrete action space!'
        super().__init__(observation_space, action_space, policy, policy_test, custom_callbacks)
        # (the form is the memory's: a wide memory has passed the wide plan for its world, and the
        # assertion below ties this agent to that world)
        if not getattr(memory, 'wide', False) and (
                self.n_states > _lib.PMA_MAX_STATES or self.n_actions > _lib.PMA_MAX_ACTIONS):
            raise NotImplementedError(
                'PMA: %d states and %d actions — this version serves worlds of up to %d states '
                'and %d actions' % (self.n_states, self.n_actions, _lib.PMA_MAX_STATES,
                                    _lib.PMA_MAX_ACTIONS))
        self.callbacks = CallbacksPMA(self, custom_callbacks)
        self.learning_rate = learning_rate
        self.gamma = gamma
        self.M = memory
        assert (memory.nb_states, memory.nb_actions) == (self.n_states, self.n_actions), \
            'the memory was built for another world'
        self._q = None
        self._q_host = np.zeros((self.n_states, self.n_actions))
        self._last = None

    # -- tables ---------------------------------------------------------------------------------
    def _alloc_tables(self) -> None:
        self._q = torch.zeros((self.n_envs, self.n_states, self.n_actions), dtype=torch.float64,
                              device=self.device)
        self._q.copy_(torch.as_tensor(self._q_host, device=self.device).expand_as(self._q))
        self._last = torch.full((self.n_envs,), -1, dtype=torch.int32, device=self.device)
        self.M._bind(self.n_envs, self.device)

    @property
    def Q(self):
        """``(S, A)`` float64 NumPy snapshot for one instance, the device tensor ``[N, S, A]``
        when vectorised.  Assigning broadcasts to all instances."""
        if self._q is None:
            return self._q_host
        return self._q[0].cpu().numpy() if self.n_envs == 1 else self._q

    @Q.setter
    def Q(self, value) -> None:
        if self._q is None:
            v = np.array(value, dtype=np.float64)
            shape = (self.n_states, self.n_actions)
            self._q_host = v.reshape(shape if v.size == shape[0] * shape[1] else (-1,) + shape)
        else:
            v = value if torch.is_tensor(value) else torch.as_tensor(
                np.asarray(value, dtype=np.float64))
            v = v.to(device=self.device, dtype=torch.float64)
            self._q.copy_(v.expand_as(self._q) if v.dim() == 2 else v)

    def predict_on_batch(self, batch):
        idx = np.array(batch).astype(int)
        if self._q is None:
            return self._q_host[idx]
        if self.n_envs == 1:
            return self._q[0][torch.as_tensor(idx, device=self.device)].cpu().numpy()
        return self._q[:, torch.as_tensor(idx, device=self.device)]

    def update_q(self, update: list) -> None:
        """agent/pma.py:319-353 for a given n-step list of experiences, applied to every instance:
        for use between sessions (inside ``train`` the 1-step update is part of the trial
        kernel).  Once the agent has device tables it is one device call, ``cobel_pma_update_q``
        with the agent's learning rate and ``gamma ** k``, the same bits as the host loop below,
        which serves the agent that has not run yet."""
        if self._q is not None:
            self.M._update_q_device(self._q, update,
                                    (self.learning_rate, self.gamma, self.policy.epsilon))
            return
        q = np.array(self.Q.cpu().numpy() if torch.is_tensor(self.Q) else self.Q)
        q = q.reshape(-1, self.n_states, self.n_actions)
        # (one entry per instance in learning_rate or gamma: every instance its own table)
        n = max(len(q), np.size(self.learning_rate), np.size(self.gamma))
        assert all(np.ndim(v) == 0 or np.shape(v) == (n,) for v in (self.learning_rate, self.gamma)) \
            and len(q) in (1, n), _device.PER_INSTANCE_SHAPE
        q = np.array(np.broadcast_to(q, (n,) + q.shape[1:]))
        rates = np.broadcast_to(np.asarray(self.learning_rate), (n,)).tolist()
        gammas = np.broadcast_to(np.asarray(self.gamma), (n,)).tolist()
        for Q, learning_rate, gamma in zip(q, rates, gammas):
            future_value = np.amax(Q[update[-1]['next_state']]) * update[-1]['terminal']
            for s, step in enumerate(update):
                r, ok = 0.0, True
                for k in range(len(update) - s):
                    if update[s + k]['terminal'] == 0 and s != len(update) - 1:
                        ok = False
                        break
                    r += update[s + k]['reward'] * (gamma ** k)
                if not ok:
                    break
                td = r + future_value * (gamma ** (k + 1))
                td -= Q[step['state']][step['action']]
                Q[step['state']][step['action']] += learning_rate * td
        self.Q = q if len(q) > 1 else q.reshape(self.n_states, self.n_actions)

    # -- launch ---------------------------------------------------------------------------------
    def _launch(self, interface, pol, flags, trials_target, steps, budget, batch) -> None:
        M = self.M
        shared = M.policy is pol
        mem = M._mem(self._q, self._mask_dev, batch,
                     agent=(self.learning_rate, self.gamma, pol.epsilon))
        run = _lib.PMARun()     # (the mask, the instance count and the seed travel in `mem`)
        self._fill_run(run, interface, flags, trials_target, steps, budget)
        run.last = _lib.ptr(self._last)
        run.replay_out = _lib.ptr(self._start_records)
        run.batch = batch
        run.flags = flags | ((_lib.PMA_SHARED_POLICY << 16) if shared else 0)
        if M._held is None:
            run.alpha, run.gamma_pow1 = self.learning_rate, self.gamma ** 1
            run.epsilon = float(pol.epsilon)
        else:      # (ignored by a launch with sets: set 0's values as placeholders)
            run.alpha, run.gamma_pow1, run.epsilon = (float(v) for v in M._held['first'][7:10])
        _lib.check(_lib.lib().cobel_pma_trial(interface.handle.ptr, C.byref(mem), C.byref(run),
                                              _lib.current_stream(self.device)))

    def _replay_logs(self, logs: dict, records, batch: int) -> dict:
        if not self.callbacks.has('on_replay_end'):
            return logs
        ups = self.M.experiences(records, batch)
        logs['replay'] = ups[0] if self.n_envs == 1 else ups
        return self.callbacks.on_replay_end(logs)

    def _run(self, interface, trials: int, steps: int, batch: int, learn: bool,
             no_replay: bool) -> None:
        # (agent/pma.py:291: test() selects with self.policy as well; _policy_in puts it on
        #  STREAM_POLICY, also where it is the memory's policy object)
        pol, flags, _ = self._session_begin(interface, trials, learn,
                                            _lib.F_NO_REPLAY if no_replay else 0, self.policy)
        M = self.M
        M._session(interface.seed, interface.instance_base)
        shared = M.policy is pol
        replays = learn and not no_replay
        self._mask_dev = self._mask_bits() if self.mask_actions else None
        self._start_records = None
        if replays:
            self._start_records = torch.zeros((self.n_envs, max(batch, 1) * 24), dtype=torch.uint8,
                                              device=self.device)
        for t in range(trials):
            interface.sync_world()
            logs = self.callbacks.on_trial_begin({'trial_reward': 0, 'steps': 0,
                                                  'trial': self.current_trial, 'trial_session': t})
            self._launch(interface, pol, flags, self.current_trial + 1, steps, 0, batch)
            if shared:       # (the memory's replay below goes on where the trial's draws ended)
                pol.counter.copy_(self.inst[:, _lib.I_CTR_POLICY])
            if replays:
                logs = self._replay_logs(logs, self._start_records, batch)
                if M.offline_need == 'device':
                    M.update_sr()
                    rec = M._replay_device(self._q, self._mask_dev, batch, self._last,
                                           M._need_device(self._last), None)
                else:
                    last = self._last.cpu().numpy()
                    M.update_sr()
                    rec = M._replay_device(self._q, self._mask_dev, batch, last,
                                           M._need_rows(last), None)
                if shared:
                    self.inst[:, _lib.I_CTR_POLICY] = pol.counter
            if self.callbacks.has('on_trial_end', 'on_replay_end'):
                st = self.inst[:, _lib.I_STEP].cpu().numpy()
                rw = self._trial_reward()
                logs['steps'] = logs['step'] = int(st[0]) if self.n_envs == 1 else float(st.mean())
                logs['trial_reward'] = float(rw[0]) if self.n_envs == 1 else float(rw.mean())
            if replays:
                logs = self._replay_logs(logs, rec, batch)
            self.current_trial += 1
            logs = self.callbacks.on_trial_end(logs)
            if self.stop:
                break
        self._session_end(pol, interface)

    def train(self, interface, trials: int, steps: int, batch_size: int = 32,
              no_replay: bool = False) -> None:
        self._run(interface, trials, steps, launch_wide(batch_size, 'PMA', 'batch_size'), True,
                  bool(no_replay))

    def test(self, interface, trials: int, steps: int) -> None:
        self._run(interface, trials, steps, 0, False, True)
