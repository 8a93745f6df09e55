"""Associative DQN — ``cobel.agent.ADQN`` (agent/adqn.py:18-279) on the kernels of csrc/adqn.hip and
csrc/mlp_fit.hip, for a ``Sequence`` environment: a network predicts one value per observation, the
value itself is the action, every experience goes to an ``ADQNMemory`` and every step replays a
batch drawn from it.

Same constructor, ``train(interface, trials, steps, batch_size=32, nb_replays=1)``,
``test(interface, trials, steps)``, ``replay``, ``retrieve_v``, ``predict_on_batch`` and the
attributes ``model``, ``memory`` (also ``M``), ``action_space = Box(-inf, inf, (1,))``,
``current_trial`` and ``stop``.  Box observation spaces only.  After a session ``model`` holds the
trained weights of instance 0, as the reference's attribute does; weights assigned to it between
sessions replace those of every instance.

One lockstep step of all instances is 1 + ``nb_replays`` launches: ``cobel_adqn_step`` (Sequence
step, store, batch draw, trial bookkeeping, the row the network sees next), then the optimisation
steps.  Two paths, chosen as ``DQN._fused_loop_ok`` chooses:

* fused — the model replicates to a stack of Linear(D <= 32, 64)-ReLU-Linear(64, 64)-ReLU-
  Linear(64, 1) with Adam and MSE in float64 or float32, and ``batch_size == 32``:
  ``cobel_mlp_fit`` reads the batch in place from the memory's states through the row indices the
  draw wrote, and its ``ep_out`` is the next step's value;
* otherwise the memory kernel still stores and draws, and the batch goes through
  ``StackedTorchNetwork.train_on_device`` (the PyTorch-ROCm loop of DESIGN §4.4).

``fused_loop = False`` keeps the second path (tests compare the two).  The first value of a session
and the values of ``test()`` come from a forward pass of the same kernel (a fit call that trains
nobody) or of the stack.  ``test()`` stores nothing and replays nothing.

Sessions and callbacks are ``SequenceAgent``'s (agent/agent.py), with no launch that covers one
trial: lockstep for ``n_envs > 1`` with the trial hooks fired per session; for ``n_envs == 1`` with
any callback the reference's loop, one look at the device per step, the logs also carrying, from
``logs.update(experience)``, ``state``, ``action``, ``reward``, ``next_state`` and
``terminal = 1 - end_trial``.  A session that would read past the last trial raises the
reference's ``IndexError`` before anything is launched.  Per-trial traces ``trial_reward_trace`` and
``trial_steps_trace`` are device tensors ``[n_envs, trials]``; ``record_steps`` > 0 keeps value,
reward, end flag and the drawn indices of that many steps per instance (``recorded_steps``,
``recorded_indices``).

Seed and instance numbers are the environment's, the memory's stream is STREAM_ADQN_MEMORY: what an
instance computes depends on its global instance number only, not on ``n_envs`` and not on how a
run is cut into sessions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..memory.adqn import ADQNMemory
from ..spaces import Box
from .agent import SequenceAgent
from .dyna_dsr import DynaDSR


class ADQN(SequenceAgent):
    _who = 'ADQN'
    _row_width = 3      # value, reward, end
    one_trial_launch = False

    def __init__(self, observation_space, model, memory=None, custom_callbacks=None) -> None:
        if type(observation_space) is not Box:
            raise NotImplementedError(
                'ADQN: %s observation spaces — this version serves Box observation spaces'
                % type(observation_space).__name__)
        super().__init__(observation_space, Box(-np.inf, np.inf, (1,), np.float64),
                         custom_callbacks)
        self.shape = tuple(int(s) for s in observation_space.shape)
        self.dim = int(np.prod(self.shape))
        if not 1 <= self.dim <= _lib.RW_MAX_DIM:
            raise NotImplementedError(
                'ADQN: observations of %d components — this version serves 1 to %d components'
                % (self.dim, _lib.RW_MAX_DIM))
        self.model = model
        self.memory = ADQNMemory(observation_space) if memory is None else memory
        assert isinstance(self.memory, ADQNMemory) and self.memory.dim == self.dim, \
            'ADQN takes an ADQNMemory over its own observation space'
        self.fused_loop = None        # None: whenever the run qualifies; False: never
        self.fused_steps = 0          # lockstep steps whose replays ran in cobel_mlp_fit so far
        self._net = self._idx_trace = None      # (record_steps keeps the drawn indices as well)
        self._batch = 0

    @property
    def M(self):
        return self.memory

    # -- device state -----------------------------------------------------------------------------
    def _bind_to(self, n_envs: int, device) -> None:
        N, device = int(n_envs), torch.device(device)
        if self.n_envs is not None:
            assert self.n_envs == N, \
                'an agent stays bound to the instance count / device it first trained on'
            return
        self.n_envs, self.device = N, device
        self.model.set_device(device)
        self._net = self.model.replicate(N)
        self.dtype = next(iter(self._net.params.values())).dtype
        dev = device
        self._value = torch.zeros((N, 1, 1), dtype=self.dtype, device=dev)
        self._ep_index = torch.zeros(N, dtype=torch.int32, device=dev)
        self._active = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._alive = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._nobody = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._done = torch.zeros(N, dtype=torch.int32, device=dev)
        self._step_rec = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        self._session_buffers()

    def _batch_buffers(self, B: int) -> None:
        if B == self._batch:
            return
        N, dev = self.n_envs, self.device
        self._in_index = torch.zeros((N, B), dtype=torch.int32, device=dev)
        self._idx = torch.zeros((N, B), dtype=torch.int32, device=dev)
        self._targets = torch.zeros((N, B), dtype=self.dtype, device=dev)
        self._batch = B

    def _reserve(self, trials: int, B: int = 0) -> None:
        super()._reserve(trials)
        if self.record_steps and B and self._idx_trace is None:
            self._idx_trace = torch.full((self.n_envs, int(self.record_steps), B), -1,
                                         dtype=torch.int32, device=self.device)
        assert self._idx_trace is None or not B or self._idx_trace.shape[2] == B, \
            'record_steps keeps the indices of one batch size'

    def recorded_steps(self, instance: int = 0) -> np.ndarray:
        """Rows (value, reward, end) kept since ``record_steps`` was set."""
        return super().recorded_steps(instance)

    def recorded_indices(self, instance: int = 0) -> np.ndarray:
        """The drawn indices ``[steps, batch_size]`` of the same steps (-1 in the rows of test())."""
        n = int(self._trace_len[instance].item())
        return self._idx_trace[instance, :n].cpu().numpy()

    # -- the network ------------------------------------------------------------------------------
    def _adopt_user_weights(self) -> None:
        if not self._net.matches(self.model, 0):
            self._net.load_from(self.model)

    def _fused_ok(self, batch_size: int) -> bool:
        """The run is one ``cobel_mlp_fit`` covers: a stack of Linear(D <= 32, 64)-ReLU-
        Linear(64, 64)-ReLU-Linear(64, 1), MSE, Adam, batches of 32, float64 or float32."""
        net = self._net
        if self.fused_loop is False or not net.fused_mlp or int(batch_size) != 32 \
                or len(self.shape) != 1 or self.dtype not in (torch.float64, torch.float32):
            return False
        names = net._mlp3_names()
        if names is None or not net._fused_adam_ok() \
                or type(net.criterion) is not torch.nn.MSELoss \
                or getattr(net.criterion, 'reduction', '') != 'none':
            return False
        w = [net.params[k + '.weight'] for k in names]
        return w[0].shape[2] == self.dim and w[2].shape[1] == 1 and \
            _lib.lib().cobel_mlp_query(w[0].shape[2], w[0].shape[1], w[1].shape[1], 1, 32,
                                       int(self.dtype == torch.float64), None) == _lib.OK

    def _fit_struct(self, table):
        """cobel_mlp_fit on the drawn batch, read in place from the memory's states; its extra row
        is the observation every instance sees next."""
        net, mem = self._net, self.memory
        names = net._mlp3_names()
        self._fit_tensors = ptrs = DynaDSR._mlp_ptrs(net, names)
        steps = DynaDSR._step_counts(net)
        fit = _lib.MLPFit()
        for dst, key in ((fit.w, 'w'), (fit.b, 'b'), (fit.m_w, 'mw'), (fit.m_b, 'mb'),
                         (fit.v_w, 'vw'), (fit.v_b, 'vb')):
            for k in range(3):
                dst[k] = _lib.ptr(ptrs[key][k])
        g = net.optimizer.param_groups[0]
        fit.lr, (fit.beta1, fit.beta2) = float(g['lr']), (float(b) for b in g['betas'])
        fit.eps, fit.weight_decay, fit.tau = float(g['eps']), float(g['weight_decay']), 0.0
        fit.steps = _lib.ptr(steps)
        fit.in_table, fit.in_index = _lib.ptr(mem._arrays['states']), _lib.ptr(self._in_index)
        fit.targets = _lib.ptr(self._targets)
        fit.ep_table, fit.ep_index = _lib.ptr(table), _lib.ptr(self._ep_index)
        fit.ep_rows, fit.ep_out = 1, _lib.ptr(self._value)
        fit.in_div = fit.tgt_div = fit.act_div = fit.ep_div = 1
        fit.n, fit.n_inputs, fit.n_outputs = self.n_envs, self.dim, 1
        fit.is_float64 = int(self.dtype == torch.float64)
        return fit

    def _forward_rows(self, table) -> None:
        """``_value`` = the stack's value of row ``_ep_index`` of the observation table."""
        x = table[self._ep_index.to(torch.int64)].reshape((self.n_envs, 1) + self.shape)
        self._value.copy_(self._net.predict_on_device(x.to(self.dtype)).reshape(self.n_envs, 1, 1))

    # -- one session ------------------------------------------------------------------------------
    @staticmethod
    def _experience(interface, step: int, value: float, reward: float, end: bool) -> dict:
        """The experience of step ``step`` of the trial instance 0 stands in (agent/adqn.py:138-144),
        the observations from the host's tables: the position depends on the schedule alone."""
        t = interface.tables
        at = int(interface.step_at(0, step)[0])
        nxt = 0 if end else t['step_obs'][at + 1]      # (row 0 is the zero observation)
        shape = t['shape']
        return {'state': t['obs_table'][t['step_obs'][at]].reshape(shape).copy(), 'action': value,
                'reward': reward, 'next_state': t['obs_table'][nxt].reshape(shape).copy(),
                'terminal': 1 - int(end)}

    def _refuse(self, interface) -> None:
        if interface.has_array_rewards and not interface.overwrite:
            raise NotImplementedError(
                'ADQN: the Sequence has array rewards and overwrite=False — the reference would '
                'index the reward with int(value) (interface/sequence.py:165); this version serves '
                'array rewards with overwrite=True only')

    def _open(self, interface, trials: int, steps: int, learn: bool, batch_size: int = 0,
              nb_replays: int = 0) -> None:
        """Describe the whole session to ``cobel_adqn_step`` and compute the first value; what
        ``_launch`` then runs is ``_one_step``, one lockstep step of all instances."""
        B, nb_replays = int(batch_size), int(nb_replays)
        mem = self.memory
        mem._adopt(interface)
        self._adopt_user_weights()
        N, first = self.n_envs, self.current_trial
        self._left = left = interface.session_steps(trials, steps)
        mem.reserve(int((mem._h_count + (left if learn else 0)).max()) if learn or mem.cap else 1)
        fused = self._fused_ok(B if learn else 32)
        self._batch_buffers(B if learn else (self._batch or 32))
        if learn:       # (the traces are reserved; the drawn indices need the batch size)
            self._reserve(first + trials, B)
        self._done.zero_()
        table = interface._dev['obs_table']
        rows = interface.tables['step_obs'][interface.step_at(slice(None))[0]]
        self._ep_index.copy_(torch.as_tensor(rows.astype(np.int32), device=self.device))

        m = mem._struct()
        run = _lib.ADQNStep()
        run.value, run.in_index = _lib.ptr(self._value), _lib.ptr(self._in_index)
        run.targets, run.idx = _lib.ptr(self._targets), _lib.ptr(self._idx)
        run.ep_index, run.active, run.alive = _lib.ptr(self._ep_index), _lib.ptr(self._active), \
            _lib.ptr(self._alive)
        run.done, run.step_rec = _lib.ptr(self._done), _lib.ptr(self._step_rec)
        self._fill_session(run, first, trials, steps, 0)
        run.idx_trace = _lib.ptr(self._idx_trace) if learn else None
        run.n, run.batch, run.is_float64 = N, self._batch, int(self.dtype == torch.float64)
        run.flags = _lib.F_LEARN if learn else 0
        fit = self._fit_struct(table) if fused else None
        lib, seq, states = _lib.lib(), interface.seq, mem._arrays['states']

        def value_of_next() -> None:
            if fused:       # a fit call that trains nobody writes ep_out and nothing else
                fit.train, fit.active = _lib.ptr(self._nobody), None
                _lib.check(lib.cobel_mlp_fit(C.byref(fit), _lib.current_stream(self.device)))
            else:
                self._forward_rows(table)

        def one_step() -> None:
            st = _lib.current_stream(self.device)
            if learn:
                stored = left > 0
                m.count_min, m.count_max = int(mem._h_count.min()), int(mem._h_count.max())
            _lib.check(lib.cobel_adqn_step(C.byref(seq), C.byref(m), C.byref(run), st))
            if not learn:
                value_of_next()
                return
            mem._h_count += stored
            left[stored] -= 1
            if fused:
                fit.train, fit.active = None, _lib.ptr(self._active)
                for _ in range(nb_replays):
                    _lib.check(lib.cobel_mlp_fit(C.byref(fit), st))
                self.fused_steps += 1
                return
            batch = states.view(N * mem.cap, self.dim)[self._in_index.to(torch.int64)]
            batch = batch.reshape((N, B) + self.shape).to(self.dtype)
            active = self._active.bool()
            for _ in range(nb_replays):
                self._net.train_on_device(batch, self._targets[..., None], active)
            self._forward_rows(table)

        value_of_next()
        self._one_step = one_step

    def _launch(self, interface, pol, learn: bool, first: int, trials: int, steps: int,
                budget: int) -> None:
        for _ in range(1 if budget else int(self._left.max()) if self.n_envs else 0):
            self._one_step()

    def _step_logs(self, interface, step: int) -> tuple:
        value, reward, end, _ = self._step_rec[0].cpu().numpy()
        return self._experience(interface, step, float(value), float(reward), bool(end)), \
            float(reward), end

    def _after_trial(self, logs=None):
        self._net.write_back(self.model, 0)
        return logs

    # -- reference surface ------------------------------------------------------------------------
    def train(self, interface, trials: int, steps: int, batch_size: int = 32,
              nb_replays: int = 1) -> None:
        assert int(batch_size) > 0 and int(nb_replays) > 0
        self._session(interface, trials, steps, True, batch_size=batch_size, nb_replays=nb_replays)

    def test(self, interface, trials: int, steps: int) -> None:
        self._session(interface, trials, steps, False)

    def replay(self, batch_size: int = 32, nb_replays: int = 1) -> None:
        """agent/adqn.py:221-236: one batch from the memory, ``nb_replays`` optimisation steps."""
        assert batch_size > 0
        assert nb_replays > 0
        mem = self.memory
        if self.n_envs is None:
            mem.reserve(0)
            self._bind_to(mem.n_envs, mem.device)
        self._adopt_user_weights()
        _, rows, targets = mem._draw(batch_size, self.dtype)
        batch = mem._arrays['states'].view(self.n_envs * mem.cap, self.dim)[rows.to(torch.int64)]
        batch = batch.reshape((self.n_envs, int(batch_size)) + self.shape).to(self.dtype)
        for _ in range(int(nb_replays)):
            self._net.train_on_device(batch, targets[..., None])
        self._net.write_back(self.model, 0)

    def predict_on_batch(self, batch):
        """agent/adqn.py:261-279: ``[B, 1]`` for one instance, the device tensor ``[n_envs, B, 1]``
        when vectorised (the same batch for every instance)."""
        if self._net is None:
            return self.model.predict_on_batch(batch)
        self._adopt_user_weights()
        b = torch.as_tensor(batch if torch.is_tensor(batch) else np.asarray(batch),
                            device=self.device).to(self.dtype)
        out = self._net.predict_on_device(b[None].expand(self.n_envs, *b.shape).contiguous())
        return out[0].cpu().numpy() if self.n_envs == 1 else out

    def retrieve_v(self, state):
        """agent/adqn.py:238-259: ``[1]`` for one instance, ``[n_envs, 1]`` when vectorised."""
        s = state.detach().cpu().numpy() if torch.is_tensor(state) else np.asarray(state)
        out = self.predict_on_batch(s[None])
        return out.flatten() if isinstance(out, np.ndarray) else out[:, 0]
