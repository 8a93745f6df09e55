"""ADQN memory — ``cobel.memory.ADQNMemory`` (memory/adqn.py:29-198) on the kernels of
csrc/adqn.hip: every experience is kept, and a replay batch is drawn with recency-decayed
prediction-error priorities.

``ADQNMemory(observation_space, decay=1.0, rpe=True, rng=None)`` as in the reference, plus
``n_envs``, ``seed``, ``device`` and ``instance_base`` as the environments have them.  Box
observation spaces only (1 to 64 components); ``Dict`` and ``Tuple`` spaces raise
``NotImplementedError``, as ``Sequence`` does.

``states``, ``reinforcements``, ``errors`` and ``priorities``: with ``n_envs == 1`` NumPy arrays of
the reference's shapes, ``(count,) + shape`` and ``(count,)``.  Vectorised they are device tensors
``[n_envs, max(count), ...]`` PADDED behind every instance's own ``count`` (a device tensor
``[n_envs]``); what lies behind an instance's count is not part of its memory.  ``decay`` and
``rpe`` are read at every call.

``store(experience)`` reads ``state``, ``action`` and ``reward`` (one experience, or one per
instance: ``state [n_envs, ...]``, ``action`` and ``reward [n_envs]``); ``sample_batch(batch_size)``
returns ``(observations, rewards)`` — ``[B, ...]`` and ``[B]`` NumPy arrays for one instance, device
tensors ``[n_envs, B, ...]`` and ``[n_envs, B]`` otherwise; the indices stay in ``last_indices``.
Both are one launch.  The draws are ``batch_size`` doubles of ONE call of the instance's stream
STREAM_ADQN_MEMORY (counter = calls so far, sub = position in the batch): what
``TapeRNG(seed, g, 7).choice(n, p=probs, size=batch_size)`` hands the reference.  The cumulative
distribution is summed in the fixed order DESIGN.md §4.1k writes down.

Capacity grows on the host between calls by amortised doubling (allocate, copy, swap);
``reserve(count)`` makes room ahead of a session, whose need is known before its first launch.
The host keeps a mirror of the counts (they follow from the calls alone), so a store into a full
memory and a draw from an empty one are refused before anything is launched — the latter with the
``ValueError`` of the reference's ``Generator.choice``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..interface.gridworld import _as_seed
from ..spaces import Box


class ADQNMemory:
    def __init__(self, observation_space, decay: float = 1.0, rpe: bool = True, rng=None,
                 n_envs: int = 1, seed: int | None = None, device=None,
                 instance_base: int = 0) -> None:
        assert 0 <= decay <= 1
        if type(observation_space) is not Box:
            raise NotImplementedError(
                'ADQNMemory: %s observation spaces — this version serves Box observation spaces'
                % type(observation_space).__name__)
        self.shape = tuple(int(s) for s in observation_space.shape)
        self.dim = int(np.prod(self.shape))
        if not 1 <= self.dim <= _lib.RW_MAX_DIM:
            raise NotImplementedError(
                'ADQNMemory: observations of %d components — this version serves Box observations '
                'of 1 to %d components' % (self.dim, _lib.RW_MAX_DIM))
        assert int(n_envs) >= 1
        self.rng = rng
        self.decay: float = decay
        self.rpe: bool = rpe
        self.n_envs = int(n_envs)
        self.seed = (int(seed) & 0xFFFFFFFFFFFFFFFF) if seed is not None else \
            (None if rng is None else _as_seed(rng))
        self.device = None if device is None else torch.device(device)
        self.instance_base = int(instance_base)
        self.instance_ids = None
        self.cap = 0
        self.last_indices = None
        self._h_count = np.zeros(self.n_envs, dtype=np.int64)
        self._arrays = None

    # -- device state -----------------------------------------------------------------------------
    def _adopt(self, interface) -> None:
        """Take instance count, device, seed and instance numbers from the environment the agent
        meets: all streams of an instance derive from the environment's seed."""
        N, dev = int(interface.n_envs), torch.device(interface.device)
        same = self.device is not None and self.device.type == dev.type and \
            self.device.index in (None, dev.index)
        if not self._h_count.any() and (N != self.n_envs or not same or self._arrays is None):
            # (an empty memory follows the environment; the draw counters start with it)
            self._arrays, self.cap = None, 0
            self.n_envs, self.device, same = N, dev, True
            self._h_count = np.zeros(N, dtype=np.int64)
        assert self.n_envs == N and same, \
            'the memory holds %d instances on %s, the environment %d on %s' % (
                self.n_envs, self.device, N, dev)
        if self.seed is None:
            self.seed = interface.seed
        assert self.seed == interface.seed, \
            'all streams of an instance derive from the environment seed'
        self.instance_base, self.instance_ids = interface.instance_base, interface.instance_ids

    def _alloc(self, cap: int) -> dict:
        N, D, dev = self.n_envs, self.dim, self.device
        assert N * cap < 2 ** 31, \
            'ADQNMemory: %d instances of capacity %d (their product must stay below 2^31)' % (N, cap)
        f = dict(dtype=torch.float64, device=dev)
        return {'states': torch.zeros((N, cap, D), **f), 'reinforcements': torch.zeros((N, cap), **f),
                'errors': torch.zeros((N, cap), **f), 'priorities': torch.zeros((N, cap), **f),
                'scratch': torch.zeros((N, cap), **f)}

    def reserve(self, count: int) -> None:
        """Room for ``count`` experiences per instance: amortised doubling, on the host."""
        count = int(count)
        if self.device is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if self.seed is None:
            self.seed = _as_seed(None)
        if self._arrays is not None and count <= self.cap:
            return
        cap = max(count, 2 * self.cap, 16)
        new = self._alloc(cap)
        if self._arrays is None:
            self._count = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
            self._draw_ctr = torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        else:
            for k in ('states', 'reinforcements', 'errors', 'priorities'):
                new[k][:, :self.cap] = self._arrays[k]
        self._arrays, self.cap = new, cap

    def _struct(self):
        a = self._arrays
        m = _lib.ADQNMem()
        m.states, m.reinforcements = _lib.ptr(a['states']), _lib.ptr(a['reinforcements'])
        m.errors, m.priorities = _lib.ptr(a['errors']), _lib.ptr(a['priorities'])
        m.scratch = _lib.ptr(a['scratch'])
        m.count, m.draw_ctr = _lib.ptr(self._count), _lib.ptr(self._draw_ctr)
        m.instance_ids = _lib.ptr(self.instance_ids)
        m.n, m.dim, m.cap = self.n_envs, self.dim, self.cap
        m.count_min, m.count_max = int(self._h_count.min()), int(self._h_count.max())
        m.instance_base, m.flags = self.instance_base, _lib.ADQN_RPE if self.rpe else 0
        assert 0 <= self.decay <= 1
        m.decay, m.seed = float(self.decay), self.seed
        return m

    # -- the reference's attributes ---------------------------------------------------------------
    def _view(self, key: str):
        tail = self.shape if key == 'states' else ()
        if self._arrays is None:
            if self.n_envs == 1:
                return np.zeros((0,) + tail)
            return torch.zeros((self.n_envs, 0) + tail, dtype=torch.float64, device=self.device)
        top = int(self._h_count.max())
        t = self._arrays[key][:, :top].reshape((self.n_envs, top) + tail)
        return t[0].cpu().numpy() if self.n_envs == 1 else t

    @property
    def states(self):
        return self._view('states')

    @property
    def reinforcements(self):
        return self._view('reinforcements')

    @property
    def errors(self):
        return self._view('errors')

    @property
    def priorities(self):
        return self._view('priorities')

    @property
    def count(self):
        """Experiences held: an int for one instance, the device tensor ``[n_envs]`` otherwise."""
        if self.n_envs == 1:
            return int(self._h_count[0])
        if self._arrays is None:
            return torch.zeros(self.n_envs, dtype=torch.int32, device=self.device)
        return self._count

    # -- the reference's methods ------------------------------------------------------------------
    def _per_instance(self, v, shape):
        a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
        a = np.broadcast_to(a.reshape((-1,) + shape), (self.n_envs,) + shape)
        return torch.as_tensor(np.array(a, order='C'), device=self.device)

    def store(self, experience: dict) -> None:
        """memory/adqn.py:119-138."""
        self.reserve(int(self._h_count.max()) + 1)
        state = self._per_instance(experience['state'], (self.dim,))
        action = self._per_instance(experience['action'], ())
        reward = self._per_instance(experience['reward'], ())
        m = self._struct()
        _lib.check(_lib.lib().cobel_adqn_store(C.byref(m), 1, _lib.ptr(state), _lib.ptr(action),
                                               _lib.ptr(reward), _lib.current_stream(self.device)))
        self._h_count += 1

    def _draw(self, batch_size: int, dtype=torch.float64):
        """The launch of ``sample_batch``: indices ``[n_envs, B]`` (int32), rows of ``states`` viewed
        ``[n_envs * cap, D]``, and the rewards in ``dtype``."""
        B = int(batch_size)
        assert B >= 1
        if self._arrays is None or int(self._h_count.min()) == 0:
            raise ValueError("'a' cannot be empty unless no samples are taken")
        N, dev = self.n_envs, self.device
        idx = torch.zeros((N, B), dtype=torch.int32, device=dev)
        rows = torch.zeros((N, B), dtype=torch.int32, device=dev)
        targets = torch.zeros((N, B), dtype=dtype, device=dev)
        m = self._struct()
        _lib.check(_lib.lib().cobel_adqn_sample(C.byref(m), B, int(dtype == torch.float64),
                                                _lib.ptr(idx), _lib.ptr(rows), _lib.ptr(targets),
                                                _lib.current_stream(dev)))
        self.last_indices = idx
        return idx, rows, targets

    def sample_batch(self, batch_size: int):
        """memory/adqn.py:140-164."""
        idx, rows, targets = self._draw(batch_size)
        B = idx.shape[1]
        flat = self._arrays['states'].view(self.n_envs * self.cap, self.dim)
        obs = flat[rows.to(torch.int64)].reshape((self.n_envs, B) + self.shape)
        if self.n_envs == 1:
            return obs[0].cpu().numpy(), targets[0].cpu().numpy()
        return obs, targets
