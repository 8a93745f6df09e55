"""Host-side plumbing the device memories share (``SFMAMemory``, ``PMAMemory``, ``DynaQMemory``);
``mask_bits`` also serves the agents' launchers.  Nothing here launches a kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib

NOT_BOUND = 'the memory has no device tables yet: train an agent with it, or call bind()'


class DeviceMemory:
    """``bind()`` / ``_session()`` of a memory whose tables live on the device.  The class itself
    brings ``_bind(n_envs, device)``, a no-op on a bound memory, which sets ``counter``."""

    _is_bound = property(lambda self: self.counter is not None)

    def bind(self, n_envs: int = 1, device=None, seed: int = 0, instance_base: int = 0) -> None:
        """Put the tables of ``n_envs`` instances on ``device`` (default: the current GPU) for a
        memory that is used without an agent; instance i draws from the streams of
        (``seed``, ``instance_base + i``)."""
        assert not self._is_bound, 'the memory is bound already'
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self._bind(n_envs, torch.device(device))
        self._session(seed, instance_base)

    def _session(self, seed: int, instance_base: int, n_worlds: int = 1) -> None:
        self.seed, self.instance_base, self._n_worlds = int(seed), int(instance_base), int(n_worlds)


PER_INSTANCE_SHAPE = 'per-instance hyper-parameters need one entry per environment instance'


def param_columns(values, n: int):
    """Scalars or [N] arrays -> float64 arrays, or None if every one of them is a scalar; an
    array of another shape is an ``AssertionError``."""
    vals = [np.asarray(v, dtype=np.float64) for v in values]
    if all(v.ndim == 0 for v in vals):
        return None
    for v in vals:
        assert v.ndim == 0 or v.shape == (n,), PER_INSTANCE_SHAPE
    return np.stack([np.broadcast_to(v, (n,)) for v in vals], axis=1)


def param_sets(cols, key, fill, device):
    """Per-instance parameter columns [N, K] as parameter sets: the distinct rows become sets
    (``fill(rows)`` -> a ctypes array of them), every instance gets the uint16 index of its row.
    Returns ``(key, sets, index, number of sets, row of set 0)`` with the two device tensors, or
    None if the bytes of the columns are ``key``, those of the tensors the caller holds."""
    new = cols.tobytes()
    if new == key:
        return None
    uniq, inv = np.unique(cols, axis=0, return_inverse=True)
    assert len(uniq) <= 65535, 'at most 65535 distinct parameter combinations per launch'
    raw = np.frombuffer(fill(uniq), dtype=np.uint8).copy()
    index = np.ascontiguousarray(inv.reshape(-1).astype(np.uint16)).view(np.int16)
    return (new, torch.as_tensor(raw, device=device), torch.as_tensor(index, device=device),
            len(uniq), uniq[0])


def plan4(entry, *args):
    """The four ints a ``cobel_*_plan`` entry point writes, as the ctypes array."""
    out = (C.c_int32 * 4)()
    _lib.check(entry(*args, C.byref(out)))
    return out


def per_instance(value, n: int, name: str, limit: int, none_as=None):
    """scalar / [N] -> int32 [N], range-checked against ``[0, limit)``.  ``none_as=None``: None
    stays None and a negative entry is an ``IndexError``; ``none_as=-1``: None (the value or an
    entry of a list) and negative entries become -1."""
    if value is None and none_as is None:
        return None
    if value is None or isinstance(value, (list, tuple)):
        value = none_as if value is None else [none_as if v is None else v for v in value]
    a = np.array(np.broadcast_to(np.asarray(value, dtype=np.int64), (n,)))
    if (a >= limit).any() or (none_as is None and (a < 0).any()):
        raise IndexError('%s outside [0, %d)' % (name, limit))
    a[a < 0] = -1
    return np.ascontiguousarray(a, dtype=np.int32)


def records(experience: dict, n: int, dtype, limits: dict, none_as=None, skip=()):
    """An experience dictionary of scalars (every instance gets the same) or [N] arrays as a record
    array [N] of ``dtype``: the fields named in ``limits`` go through ``per_instance``,
    ``nonterminal`` is ``experience['terminal'] != 0``, the others are broadcast from the entry of
    their name; the fields in ``skip`` stay zero."""
    rec = np.zeros(n, dtype=dtype)
    for name in dtype.names:
        if name in limits:
            rec[name] = per_instance(experience[name], n, name, limits[name], none_as)
        elif name == 'nonterminal':
            rec[name] = np.broadcast_to(np.asarray(experience['terminal']), (n,)) != 0
        elif name not in skip:
            rec[name] = np.broadcast_to(np.asarray(experience[name]), (n,))
    return rec


def squeeze(a):
    """[1, ...] -> [...]: one instance looks like the reference's table."""
    return a[0] if a.shape[0] == 1 else a


class PackedModel:
    """The reference's ``rewards`` / ``states`` / ``terminals`` of a memory whose ``table`` holds
    packed model records (int64 [N, S, 4]: float32 reward estimate, next state, nonterminal)."""

    _squeeze = staticmethod(squeeze)

    def _decode(self):
        raw = self.table.cpu().numpy()
        lo = (raw & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        hi = (raw >> 32) & 0xFFFFFFFF
        return lo, (hi & 0xFFFF).astype(np.int64), ((hi >> 16) & 1).astype(np.int64)

    rewards = property(lambda self: squeeze(self._decode()[0]))
    states = property(lambda self: squeeze(self._decode()[1]))
    terminals = property(lambda self: squeeze(self._decode()[2]))


def mask_bits(mask, n_states: int, n_actions: int):
    """Boolean action mask [S, A] -> one bit per action: a uint8 per state up to eight actions, a
    32-bit word (as int32) beyond (cobel_hip.h)."""
    m = np.asarray(mask, dtype=bool).reshape(n_states, n_actions)
    assert m.any(axis=1).all(), 'The action mask masks all actions!'
    bits = (m * (1 << np.arange(n_actions, dtype=np.int64))).sum(axis=1)
    if n_actions <= 8:
        return bits.astype(np.uint8)
    return bits.astype(np.uint32).view(np.int32)
