"""MFEC agent — ``cobel.agent.MFEC`` (agent/mfec.py:239-559): Model-Free Episodic Control
(Blundell et al. 2016) on the kernels of csrc/mfec.hip.

Same constructor, ``train(interface, trials, steps=32)``, ``test``, ``predict_on_batch``,
``retrieve_q``, ``process_observation`` and attributes (``capacity``, ``k``, ``gamma``, ``model``,
``projection_size``, ``projection``, ``rng``, ``Q``).  The environment is a ``Topology`` (poses or
an ``OfflineSimulator``'s pre-rendered observations): its observation is a function of the node, so
at first contact the host builds the feature table ``F[S, D]`` — row by row with the reference's own
expression, ``np.dot(obs.flatten(), projection)``, or one ``model.predict_on_batch`` per node — and
``cobel_mfec_pairs`` turns it into the two S x S tables the kernels search with.  The per-action
memories hold node ids and live on the device; ``Q.buffers[a]`` reads one back as ``ids``,
``values``, ``times`` (and ``states``, the feature rows, as the reference stores them).

Time stamps are a per-instance counter that advances by one per training step where the reference
stamps ``time.time()``: only their order matters.  Among equidistant entries the order is that of a
scikit-learn ``KDTree`` of a single leaf ("MFEC").
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..spaces import Box, Dict, Discrete
from .agent import FusedAgent


class ActionBufferView:
    """One action's memory of one instance, read back: ``ids`` (node per entry), ``values``,
    ``times``; ``states`` are the entries' feature rows."""

    def __init__(self, ids, values, times, features, capacity) -> None:
        self.ids, self.values, self.times, self.capacity = ids, values, times, capacity
        self._features = features

    @property
    def states(self):
        return [self._features[i] for i in self.ids]

    def __len__(self) -> int:
        return len(self.ids)

    def __iter__(self):
        return iter((self.ids, self.values, self.times))


class QECView:
    def __init__(self, buffers, k) -> None:
        self.buffers, self.k = tuple(buffers), k


class MFEC(FusedAgent):
    general_actions = True

    def __init__(self, observation_space, action_space, policy, policy_test=None,
                 capacity: int = 2000, k: int = 3, gamma: float = 0.97, model=None,
                 projection_size: int = 256, custom_callbacks=None, rng=None) -> None:
        assert type(action_space) is Discrete, 'Wrong action space!'
        super().__init__(observation_space, action_space, policy, policy_test, custom_callbacks)
        self.rng = np.random.default_rng() if rng is None else rng
        self.capacity = capacity
        self.nb_actions = int(action_space.n)
        self.k = k
        self.gamma = gamma
        self.model = model
        self.projection_size = projection_size
        if self.nb_actions > _lib.MFEC_MAX_ACTIONS:
            raise NotImplementedError('MFEC: %d actions — this version serves 1 to %d actions'
                                      % (self.nb_actions, _lib.MFEC_MAX_ACTIONS))
        if not 1 <= int(capacity) <= _lib.MFEC_MAX_CAPACITY:
            raise NotImplementedError('MFEC: capacity %d — this version serves a capacity of 1 to %d'
                                      % (capacity, _lib.MFEC_MAX_CAPACITY))
        if not 1 <= int(k) <= _lib.MFEC_MAX_K:
            raise NotImplementedError('MFEC: k = %d — this version serves k of 1 to %d'
                                      % (k, _lib.MFEC_MAX_K))
        if type(self.observation_space) is Box:
            self.projection = self.rng.random(
                (int(np.prod(self.observation_space.shape)), self.projection_size))
        elif type(self.observation_space) is Dict:
            units = 0
            for _, space in self.observation_space.items():
                assert type(space.shape) is tuple
                units += int(np.prod(space.shape))
            self.projection = self.rng.random((units, self.projection_size))
        self.features = None          # F[S, D], built at first contact with an environment
        self.record_steps = 0         # > 0: keep that many steps' (state, action, reward, end, q)
        self._mem = self._trace = self._trace_len = self._episode = None

    # -- features ---------------------------------------------------------------------------------
    def process_observation(self, observation) -> np.ndarray:
        """agent/mfec.py:362-403."""
        if self.model is not None:
            if type(observation) is np.ndarray:
                prediction = self.model.predict_on_batch(np.array([observation]))
            elif type(observation) is list:
                prediction = self.model.predict_on_batch([np.array([o]) for o in observation])
            else:
                assert type(observation) is dict
                prediction = self.model.predict_on_batch(
                    {m: np.array([o]) for m, o in observation.items()})
            if torch.is_tensor(prediction):
                prediction = prediction.detach().cpu().numpy()
            return np.asarray(prediction).flatten()
        if type(observation) is np.ndarray:
            return np.dot(observation.flatten(), self.projection)
        if type(observation) is list:
            return np.dot(np.array(observation).flatten(), self.projection)
        assert type(observation) is dict
        return np.dot(np.array(list(observation.values())).flatten(), self.projection)

    @staticmethod
    def node_observations(interface) -> list:
        """The observation of every node of a Topology, in node order, as ``step`` returns it."""
        if getattr(interface, 'simulator', None) is not None:
            return [interface.simulator.get_observation(tuple(interface.nodes[n]['pose']))
                    for n in interface.ids]
        return [np.array(p) for p in interface.pose]

    def feature_table(self, interface) -> np.ndarray:
        """``F[S, D]``: ``process_observation`` of every node's observation, row by row."""
        rows = [np.asarray(self.process_observation(o), dtype=np.float64)
                for o in self.node_observations(interface)]
        return np.ascontiguousarray(np.stack(rows))

    def _bind(self, interface) -> None:
        if self.inst is None:
            if not hasattr(interface, 'ids'):
                raise NotImplementedError('MFEC runs on a Topology (its observation is a function '
                                          'of the node)')
            self.features = self.feature_table(interface)
        super()._bind(interface)

    def _alloc_tables(self) -> None:
        S, A, cap, N, dev = self.n_states, self.n_actions, int(self.capacity), self.n_envs, self.device
        F = self.features
        assert F.shape[0] == S and np.isfinite(F).all(), 'the features must be finite, one row per node'
        if S > _lib.MFEC_MAX_STATES:
            raise NotImplementedError('MFEC: %d states — this version serves up to %d states'
                                      % (S, _lib.MFEC_MAX_STATES))
        if F.shape[1] > _lib.MFEC_MAX_FEATURES:
            raise NotImplementedError('MFEC: %d features — this version serves up to %d features'
                                      % (F.shape[1], _lib.MFEC_MAX_FEATURES))
        self._f_dev = torch.as_tensor(F, device=dev).contiguous()
        self._rdist = torch.zeros((S, S), dtype=torch.float64, device=dev)
        self._same = torch.zeros((S, S), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().cobel_mfec_pairs(_lib.ptr(self._f_dev), S, F.shape[1],
                                               _lib.ptr(self._rdist), _lib.ptr(self._same),
                                               _lib.current_stream(dev)))
        same = self._same.cpu().numpy().astype(bool)
        if (same & ~np.eye(S, dtype=bool)).any():
            # The reference's update() replaces a stored state by one that is merely allclose to it
            # WITHOUT rebuilding its tree (agent/mfec.py:219-222): tree and list then disagree.  The
            # device buffers hold one id per entry; refuse the world instead of learning differently.
            q, j = np.argwhere(same & ~np.eye(S, dtype=bool))[0]
            raise NotImplementedError(
                'MFEC: the features of nodes %d and %d are allclose (rtol 1e-4, atol 1e-6): the '
                'reference would treat them as one state with a stale tree; this version serves '
                'worlds whose nodes are told apart' % (q, j))
        self._ids = torch.zeros((N, A, cap), dtype=torch.int32, device=dev)
        self._values = torch.zeros((N, A, cap), dtype=torch.float64, device=dev)
        self._times = torch.zeros((N, A, cap), dtype=torch.int32, device=dev)
        self._len = torch.zeros((N, A), dtype=torch.int32, device=dev)
        self._clock = torch.zeros((N,), dtype=torch.int32, device=dev)
        mem = _lib.MFECMem()
        mem.rdist, mem.same = _lib.ptr(self._rdist), _lib.ptr(self._same)
        mem.ids, mem.values, mem.times = _lib.ptr(self._ids), _lib.ptr(self._values), _lib.ptr(self._times)
        mem.len, mem.clock = _lib.ptr(self._len), _lib.ptr(self._clock)
        mem.n, mem.n_states, mem.n_actions, mem.capacity, mem.k = N, S, A, cap, int(self.k)
        self._mem = mem

    # -- the memory, read back ------------------------------------------------------------------------
    def memory(self, instance: int = 0) -> QECView:
        """The per-action buffers of one instance as (ids, values, times)."""
        A = self.n_actions
        if self._mem is None:
            empty = [ActionBufferView(np.zeros(0, np.int64), np.zeros(0), np.zeros(0), None,
                                      self.capacity) for _ in range(A)]
            return QECView(empty, self.k)
        lens = self._len[instance].cpu().numpy()
        ids = self._ids[instance].cpu().numpy()
        values = self._values[instance].cpu().numpy()
        times = self._times[instance].cpu().numpy()
        return QECView([ActionBufferView(ids[a, :lens[a]].astype(np.int64), values[a, :lens[a]].copy(),
                                         times[a, :lens[a]].astype(np.float64), self.features,
                                         self.capacity) for a in range(A)], self.k)

    @property
    def Q(self) -> QECView:
        """The memory of instance 0 (the only one unless vectorised; ``memory(i)`` for the others)."""
        return self.memory(0)

    def _nodes_of(self, batch) -> np.ndarray:
        """Node index of every entry of a batch: integers are node indices; anything else is an
        observation (looked up by its flattened key, exactly) or a feature row."""
        out = []
        for o in batch:
            if isinstance(o, (int, np.integer)):
                out.append(int(o))
                continue
            if type(o) is dict:
                key = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in o.values()])
            elif type(o) is list:
                key = np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in o])
            else:
                key = np.asarray(o, dtype=np.float64).reshape(-1)
            for table in (self._poses.reshape(self.n_states, -1), self.features):
                if table.shape[1] == key.shape[0]:
                    hit = np.flatnonzero((table == key).all(axis=1))
                    if len(hit):
                        out.append(int(hit[0]))
                        break
            else:
                raise KeyError('not an observation of this world\'s nodes')
        return np.array(out, dtype=np.int32)

    def predict_on_batch(self, batch):
        """agent/mfec.py:534-559 for a batch of observations (or node indices): ``[B, A]`` for one
        instance, the device tensor ``[N, B, A]`` when vectorised."""
        assert self._mem is not None, 'predict_on_batch needs the world: train or test first'
        nodes = torch.as_tensor(self._nodes_of(batch), device=self.device)
        out = torch.zeros((self.n_envs, len(nodes), self.n_actions), dtype=torch.float64,
                          device=self.device)
        _lib.check(_lib.lib().cobel_mfec_estimate(C.byref(self._mem), _lib.ptr(nodes), len(nodes),
                                                  _lib.ptr(out), _lib.current_stream(self.device)))
        return out[0].cpu().numpy() if self.n_envs == 1 else out

    def retrieve_q(self, state):
        """agent/mfec.py:405-421: the Q-values of a processed observation (a feature row)."""
        q = self.predict_on_batch([state])
        return q[0] if self.n_envs == 1 else q[:, 0]

    def recorded_steps(self, instance: int = 0) -> np.ndarray:
        """Rows (state, action, reward, end, q[0..A-1]) kept since ``record_steps`` was set."""
        n = int(self._trace_len[instance].item())
        return self._trace[instance, :n].cpu().numpy()

    # -- launch ---------------------------------------------------------------------------------
    def _launch(self, interface, pol, flags, trials_target, steps, budget, batch) -> None:
        N, dev = self.n_envs, self.device
        if self._episode is None or self._episode[0].shape[1] != steps:
            self._episode = (torch.zeros((N, steps), dtype=torch.int32, device=dev),
                             torch.zeros((N, steps), dtype=torch.float64, device=dev))
        if self.record_steps and self._trace is None:
            self._trace = torch.zeros((N, int(self.record_steps), 4 + self.n_actions),
                                      dtype=torch.float64, device=dev)
            self._trace_len = torch.zeros((N,), dtype=torch.int32, device=dev)
        run = _lib.MFECRun()
        self._fill_run(run, interface, flags, trials_target, steps, budget)
        run.ep_sa, run.ep_value = _lib.ptr(self._episode[0]), _lib.ptr(self._episode[1])
        run.trace, run.trace_len = _lib.ptr(self._trace), _lib.ptr(self._trace_len)
        run.trace_cap = int(self.record_steps) if self._trace is not None else 0
        run.flags = flags & (_lib.F_LEARN | _lib.F_TEST_STREAM)
        run.gamma, run.epsilon = float(self.gamma), float(pol.epsilon)
        _lib.check(_lib.lib().cobel_mfec_run(interface.handle.ptr, C.byref(self._mem),
                                             C.byref(run), _lib.current_stream(dev)))

    def train(self, interface, trials: int, steps: int = 32) -> None:
        self._session(interface, trials, steps, 0, True)

    def test(self, interface, trials: int, steps: int = 32) -> None:
        self._session(interface, trials, steps, 0, False)
