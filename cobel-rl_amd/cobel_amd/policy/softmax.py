"""Softmax policy — ``cobel.policy.softmax.Softmax`` (policy/softmax.py:11-88).

``get_action_probs`` / ``select_action`` evaluate on the GPU through ``cobel_softmax_n``, in float64
as the reference: the values minus their maximum, times ``beta``, ``exp``, divided by their sum in
action order; the action is ``searchsorted(cumsum(p) / cumsum(p)[-1], u, 'right')`` exactly like
``Generator.choice``.  Inputs may be one row ``v[A]`` (returns an int / ``p[A]``, as the reference)
or a batch ``v[N, A]``, A up to 8.  ``beta`` is a scalar or — for a batch, and for the instances of
a ``QAgent`` on a ``Sequence`` — one value per row / instance.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .greedy import _mask_bits
from .policy import Policy


class Softmax(Policy):
    def __init__(self, beta: float = 1.0, rng=None) -> None:
        super().__init__(rng)
        assert np.all(np.asarray(beta, dtype=np.float64) > 0.0), \
            'Inverse temperature must be non-negative!'
        self.beta = beta

    # -- helpers ----------------------------------------------------------------------------
    def _bind(self, n: int, device) -> None:
        from ..interface.gridworld import _as_seed
        if self.seed is None:
            self.seed = _as_seed(self.rng)
        if self.stream is None:
            self.stream = _lib.STREAM_POLICY
        if self.counter is None or self.counter.numel() != n or self.counter.device != device:
            self.counter = torch.zeros(n, dtype=torch.int32, device=device)

    def parameter_column(self, n: int) -> np.ndarray:
        """``beta`` as float64: one value, or one per instance."""
        b = np.asarray(self.beta, dtype=np.float64)
        assert b.ndim == 0 or b.shape == (n,), 'beta: a scalar or one value per instance (%d)' % n
        return b.reshape(-1)

    def _run(self, v, mask, u):
        device = torch.device('cuda', torch.cuda.current_device())
        vals = torch.as_tensor(np.asarray(v, dtype=np.float64) if not torch.is_tensor(v) else v)
        single = vals.dim() == 1
        A = int(vals.shape[-1])
        assert 1 <= A <= _lib.QSEQ_MAX_ACTIONS, 'up to %d actions' % _lib.QSEQ_MAX_ACTIONS
        vals = vals.reshape(-1, A).to(device=device, dtype=torch.float64).contiguous()
        n = vals.shape[0]
        bits = _mask_bits(mask, n, device, A)
        beta = torch.as_tensor(self.parameter_column(n), device=device).contiguous()
        if u is None:
            self._bind(n, device)
            u = torch.empty(n, dtype=torch.float64, device=device)
            _lib.check(_lib.lib().cobel_rng_uniform(
                _lib.ptr(self.counter), self.seed, self.stream, 0, _lib.ptr(u), n, 1,
                _lib.current_stream(device)))
        else:
            u = torch.as_tensor(u, dtype=torch.float64, device=device).reshape(n).contiguous()
        act = torch.empty(n, dtype=torch.uint8, device=device)
        probs = torch.empty((n, A), dtype=torch.float64, device=device)
        _lib.check(_lib.lib().cobel_softmax_n(
            _lib.ptr(vals), _lib.ptr(bits), _lib.ptr(u), _lib.ptr(beta), beta.numel(),
            _lib.ptr(act), _lib.ptr(probs), n, A, _lib.current_stream(device)))
        return single, act, probs

    # -- reference surface ------------------------------------------------------------------
    def select_action(self, v, mask=None, u=None):
        """Action(s) for Q-value row(s) ``v``; ``u`` injects the uniform draw(s) (tests)."""
        single, act, _ = self._run(v, mask, u)
        return int(act[0].item()) if single else act

    def get_action_probs(self, v, mask=None):
        single, _, probs = self._run(v, mask, 0.0 if np.ndim(v) == 1 else np.zeros(len(v)))
        p = probs.cpu().numpy()
        return p[0] if single else p
