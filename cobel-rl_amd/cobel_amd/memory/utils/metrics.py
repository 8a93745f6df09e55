"""State-state similarity metrics for SFMA — ``cobel.memory.utils.metrics``
(memory/utils/metrics.py:9-268 of the reference): ``Euclidean``, ``SR`` (successor
representation under the uniform policy) and ``DR`` (default representation with a low-rank
correction for walls).  Same constructors and attributes (``D``, ``update_transitions``).

A metric is an S x S float64 matrix per world; the SFMA kernel reads it from device memory (one
copy per world, shared by every instance).  ``sas`` may be the dense one-hot tensor
``world['sas']`` as in the reference, or the compact successor table ``world['next']`` ([S, 4]
integers), which avoids expanding the tensor.

``compute='host'`` (the default) is the reference's code: the LAPACK inverse on the host, ``D`` a
NumPy array that ``SFMAMemory`` uploads.  ``compute='device'`` (``SR`` and ``DR``) computes the
matrices on the GPU (``cobel_metric_sr`` / ``cobel_metric_dr``, csrc/metric.hip) from the compact
tables, for one world or a stack of worlds:

  ``sas``     one table ([S, 4], or a dense one-hot [S, 4, S] that is reduced to its compact form), or
              a list / [W, S, 4] stack of them; for ``DR``, ``invalid_transitions`` is then one list
              per world
  ``D``       a float64 tensor on ``device``, [S, S] for one table, [W, S, S] for a stack, which
              ``SFMAMemory`` hands to its kernels as it is; ``DR.D0`` is a device tensor too
              (``T_new`` and ``B`` are not kept)
  ``update_transitions()``  re-reads the tables (and ``invalid_transitions``) and rewrites ``D`` in
              place, in stream order, at the same address — for ``DR`` the Woodbury step alone, ``D0``
              is kept — so a memory that launched on ``D`` sees the edited world at its next launch
The device matrices are those of an in-place Gauss-Jordan elimination in a fixed order of
operations, not LAPACK's: they differ from the host's in the last bits (docs/MEASUREMENTS.md).
Refused with ``NotImplementedError`` (the host path serves these): rows that are distributions, a
dense ``T_default``, more than ``_lib.METRIC_MAX_RANK`` affected states in a world, more than
``_lib.METRIC_MAX_STATES`` states; ``ValueError`` for a gamma outside [0, 1).
"""
from __future__ import annotations

import abc

import numpy as np


def _check_compute(compute: str) -> str:
    if compute not in ('host', 'device'):
        raise ValueError("compute must be 'host' or 'device', not %r" % (compute,))
    return compute


def _compact_table(sas) -> np.ndarray:
    """One world's table as [S, 4] int32: a compact table as it is, a dense one-hot tensor reduced."""
    sas = np.asarray(sas)
    if sas.ndim == 3:
        if sas.shape[0] != sas.shape[2] or sas.shape[1] != 4:
            raise NotImplementedError('the device metrics serve four-action worlds: sas[S, 4, S] '
                                      "or next[S, 4]; use compute='host'")
        nxt = np.argmax(sas, axis=2)
        rows, acts = np.indices(nxt.shape)
        if not (np.all((sas == 0) | (sas == 1)) and np.all(sas[rows, acts, nxt] == 1)
                and np.all(sas.sum(axis=2) == 1)):
            raise NotImplementedError('the device metrics serve deterministic worlds; rows of sas '
                                      "that are distributions take compute='host'")
        sas = nxt
    if sas.ndim != 2 or sas.shape[1] != 4:
        raise NotImplementedError('the device metrics serve four-action worlds: sas[S, 4, S] or '
                                  "next[S, 4]; use compute='host'")
    if not np.issubdtype(sas.dtype, np.integer):
        if not np.all(sas == np.floor(sas)):
            raise NotImplementedError('a compact successor table holds integers')
    if sas.size and (sas.min() < 0 or sas.max() >= sas.shape[0]):
        raise IndexError('successor outside the world')
    return np.ascontiguousarray(sas, dtype=np.int32)


def _compact_stack(sas):
    """(tables [W, S, 4] int32, stacked?) of one table or a list / stack of tables."""
    if isinstance(sas, (list, tuple)):
        tabs, stacked = [_compact_table(t) for t in sas], True
    else:
        arr = np.asarray(sas)
        # [S, 4] and [S, 4, S] are one world; [W, S, 4] is a stack (a one-hot [4, 4, 4] is one world)
        stacked = arr.ndim == 3 and arr.shape[2] == 4 and not (
            arr.shape[1] == 4 and arr.shape[0] == 4 and not np.issubdtype(arr.dtype, np.integer))
        tabs = [_compact_table(t) for t in arr] if stacked else [_compact_table(arr)]
    if len(tabs) == 0 or any(t.shape != tabs[0].shape for t in tabs):
        raise ValueError('a stack of worlds holds at least one table, all of one size')
    return np.ascontiguousarray(np.stack(tabs)), stacked


class _DeviceTables:
    """What the device forms of ``SR`` and ``DR`` share: the device, the tables, ``D``."""

    def _device_setup(self, device, gamma: float, before_alloc=None) -> None:
        """Checks on the host first (``before_alloc``: a subclass's own), then the device tensors."""
        import torch
        from ... import _lib
        if not 0.0 <= float(gamma) < 1.0:
            raise ValueError('gamma = %r: the device metrics take gamma in [0, 1) (the elimination '
                             'without pivoting rests on diagonal dominance)' % (gamma,))
        tabs, self._stacked = _compact_stack(self.sas)
        if tabs.shape[1] > _lib.METRIC_MAX_STATES:
            raise NotImplementedError("%d states: the device metrics serve up to %d; use "
                                      "compute='host'" % (tabs.shape[1], _lib.METRIC_MAX_STATES))
        self._n_worlds = tabs.shape[0]
        self.version = 0      # counts update_transitions(): SFMAMemory refreshes what it expanded
        if before_alloc is not None:
            before_alloc(tabs)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        self._next = torch.as_tensor(tabs, device=self.device)
        W, S = tabs.shape[0], tabs.shape[1]
        self._D = torch.empty((W, S, S), dtype=torch.float64, device=self.device)
        self.D = self._D if self._stacked else self._D[0]

    def _reload_tables(self) -> None:
        import torch
        tabs, stacked = _compact_stack(self.sas)
        if stacked != self._stacked or tabs.shape != tuple(self._next.shape):
            raise ValueError('update_transitions(): the tables changed their shape')
        self._next.copy_(torch.as_tensor(tabs))
        self.version += 1

    def _sr_into(self, nxt, D, gamma: float) -> None:
        from ... import _lib
        _lib.check(_lib.lib().cobel_metric_sr(_lib.ptr(nxt), nxt.shape[0], nxt.shape[1],
                                              float(gamma), _lib.ptr(D),
                                              _lib.current_stream(self.device)))


def _uniform_policy_matrix(sas) -> np.ndarray:
    """``np.sum(sas, axis=1) / sas.shape[1]`` for either form of the transition table."""
    sas = np.asarray(sas)
    if sas.ndim == 3:
        return np.sum(sas, axis=1) / sas.shape[1]
    assert sas.ndim == 2, 'expected sas[S, A, S] or next[S, A]'
    n, acts = sas.shape
    T = np.zeros((n, n))
    rows = np.arange(n)
    for a in range(acts):
        np.add.at(T, (rows, sas[:, a].astype(np.int64)), 1.0)
    return T / acts


class Metric(abc.ABC):
    def __init__(self) -> None:
        self.D: np.ndarray

    @abc.abstractmethod
    def update_transitions(self) -> None:
        """Recompute the metric after the environment changed."""


class Euclidean(Metric):
    """D[s1, s2] = exp(-euclidean distance of the grid cells) (metrics.py:28-61)."""

    def __init__(self, width: int, height: int) -> None:
        super().__init__()
        rows, cols = np.divmod(np.arange(width * height), width)
        d2 = (rows[:, None] - rows[None, :]) ** 2 + (cols[:, None] - cols[None, :]) ** 2
        self.D = np.exp(-np.sqrt(d2))

    def update_transitions(self) -> None:
        pass


class SR(Metric, _DeviceTables):
    """(I - gamma T)^-1 with T the uniform-policy transition matrix (metrics.py:63-105)."""

    def __init__(self, sas, gamma: float, compute: str = 'host', device=None) -> None:
        super().__init__()
        self.sas = sas
        self.gamma = gamma
        self.compute = _check_compute(compute)
        if self.compute == 'device':
            self._device_setup(device, gamma)
            self._sr_into(self._next, self._D, gamma)
        else:
            self.update_transitions()

    def update_transitions(self) -> None:
        if self.compute == 'device':
            self._reload_tables()
            self._sr_into(self._next, self._D, self.gamma)
            return
        T = _uniform_policy_matrix(self.sas)
        self.D = np.linalg.inv(np.eye(T.shape[0]) - self.gamma * T)


class DR(Metric, _DeviceTables):
    """Default representation (metrics.py:107-268): the SR of the wall-free grid, ``D0``,
    corrected for the rows of the states that invalid transitions start from by the Woodbury
    identity, ``D = D0 - D0[:, J] (I + delta D0[:, J])^-1 delta D0``."""

    def __init__(self, width: int, height: int, sas, gamma: float, invalid_transitions,
                 T_default=None, compute: str = 'host', device=None) -> None:
        super().__init__()
        self.width, self.height = width, height
        self.nb_states = width * height
        self.sas = sas
        self.gamma = gamma
        self.invalid_transitions = invalid_transitions
        self.compute = _check_compute(compute)
        if self.compute == 'device':
            self._device_init(T_default, device)
            return
        if T_default is None:
            self.build_default_transition_matrix()
        else:
            self.T_default = T_default
        self.D0 = np.linalg.inv(np.eye(self.nb_states) - self.gamma * self.T_default)
        self.update_transitions()

    def _device_init(self, T_default, device) -> None:
        import torch
        if T_default is not None:
            raise NotImplementedError("a dense T_default takes compute='host': the device form "
                                      'builds the open field of width x height itself')

        def check(tabs):
            if tabs.shape[1] != self.nb_states:
                raise ValueError('the tables hold %d states, width x height is %d'
                                 % (tabs.shape[1], self.nb_states))
            self._affected()      # (a rank above the limit is refused before anything is computed)
        self._device_setup(device, self.gamma, check)
        self._next_default = torch.as_tensor(self.default_table(), device=self.device)
        self.D0 = torch.empty((self.nb_states, self.nb_states), dtype=torch.float64,
                              device=self.device)
        self._sr_into(self._next_default[None], self.D0[None], self.gamma)
        self._work = None
        self._woodbury()

    def default_table(self) -> np.ndarray:
        """Compact successor table of the open field (moves clamp at the border), [S, 4] int32."""
        w, h = self.width, self.height
        rows, cols = np.divmod(np.arange(self.nb_states), w)
        nxt = np.stack([rows * w + np.maximum(0, cols - 1), np.maximum(0, rows - 1) * w + cols,
                        rows * w + np.minimum(w - 1, cols + 1),
                        np.minimum(h - 1, rows + 1) * w + cols], axis=1)
        return np.ascontiguousarray(nxt, dtype=np.int32)

    def _affected(self):
        """Per world the sorted states invalid transitions start from: J [W][kmax], rank [W]."""
        from ... import _lib
        W = self._n_worlds
        lists = self.invalid_transitions if self._stacked else [self.invalid_transitions]
        if len(lists) != W:
            raise ValueError('invalid_transitions: one list per world (%d worlds, %d lists)'
                             % (W, len(lists)))
        Js = [np.unique(np.array(inv)[:, 0]).astype(np.int32) if len(inv) > 0
              else np.zeros(0, dtype=np.int32) for inv in lists]
        rank = np.array([len(j) for j in Js], dtype=np.int32)
        kmax = int(rank.max())
        if kmax > _lib.METRIC_MAX_RANK:
            raise NotImplementedError(
                "%d states are affected by invalid transitions in one world; the device form of DR "
                "serves up to %d (the rank of the Woodbury correction); use compute='host'"
                % (kmax, _lib.METRIC_MAX_RANK))
        J = np.zeros((W, kmax), dtype=np.int32)
        for w, j in enumerate(Js):
            J[w, :len(j)] = j
        return J, rank, kmax

    def _woodbury(self) -> None:
        import torch
        from ... import _lib
        J, rank, kmax = self._affected()
        W, S = self._next.shape[0], self.nb_states
        need = _lib.metric_work_bytes(W, S, kmax)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        # (the call copies J and rank in stream order: the last two calls' arrays are kept alive)
        self._host_args = (getattr(self, '_host_args', ()) + ((J, rank),))[-2:]
        _lib.check(_lib.lib().cobel_metric_dr(
            _lib.ptr(self.D0), _lib.ptr(self._next), _lib.ptr(self._next_default),
            J.ctypes.data if kmax else None, rank.ctypes.data, kmax, W, S, float(self.gamma),
            _lib.ptr(self._D), _lib.ptr(self._work), self._work.numel(),
            _lib.current_stream(self.device)))

    def update_transitions(self) -> None:
        if self.compute == 'device':
            self._reload_tables()
            self._woodbury()
            return
        self.T_new = _uniform_policy_matrix(self.sas)
        self.B = np.zeros(self.T_new.shape)
        if len(self.invalid_transitions) > 0:
            self.states = np.unique(np.array(self.invalid_transitions)[:, 0])
            eye = np.eye(self.nb_states)
            delta = (eye - self.gamma * self.T_new)[self.states] \
                - (eye - self.gamma * self.T_default)[self.states]
            cols = self.D0[:, self.states]
            alpha = np.linalg.inv(np.eye(self.states.shape[0]) + np.matmul(delta, cols))
            self.B = np.matmul(np.matmul(cols, alpha), np.matmul(delta, self.D0))
        self.D = self.D0 - self.B

    def build_default_transition_matrix(self) -> None:
        """Uniform-policy transitions of the open field (moves clamp at the border)."""
        n, w, h = self.nb_states, self.width, self.height
        rows, cols = np.divmod(np.arange(n), w)
        self.T_default = np.zeros((n, n))
        for r, c in ((rows, np.maximum(0, cols - 1)), (np.maximum(0, rows - 1), cols),
                     (rows, np.minimum(w - 1, cols + 1)), (np.minimum(h - 1, rows + 1), cols)):
            np.add.at(self.T_default, (np.arange(n), r * w + c), 0.25)
