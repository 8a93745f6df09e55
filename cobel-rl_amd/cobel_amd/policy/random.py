"""Random policy — ``cobel.policy.random.RandomDiscrete`` (policy/random.py:13-75).

``select_action`` is the reference's ``int(rng.integers(actions))``: ONE bounded integer draw of the
policy's stream, whatever the values and the mask (the reference ignores both), evaluated through
``cobel_policy_select_n``; ``get_action_probs`` returns ``full(actions, 1 / actions)``.  One row
``v[A]`` (returns an int) or a batch ``v[N, A]``.  The reference's ``RandomUniform`` and
``RandomGaussian`` return continuous actions, which no interface here takes: they are not ported.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .greedy import select_n
from .policy import Policy


class RandomDiscrete(Policy):
    def __init__(self, actions: int, rng=None) -> None:
        super().__init__(rng)
        assert actions > 0, 'There must be at least one action!'
        self.actions = int(actions)

    def _bind(self, n: int, device) -> None:
        from ..interface.gridworld import _as_seed
        if self.seed is None:
            self.seed = _as_seed(self.rng)
        if self.stream is None:
            self.stream = _lib.STREAM_POLICY
        if self.counter is None or self.counter.numel() != n or self.counter.device != device:
            self.counter = torch.zeros(n, dtype=torch.int32, device=device)

    def select_action(self, v, mask=None, k=None):
        """Random action(s), one per row of ``v``; ``k`` injects the 32-bit word(s) of the bounded
        draw(s) (tests): the action is ``(k * actions) >> 32``."""
        device = torch.device('cuda', torch.cuda.current_device())
        A = self.actions
        assert A <= _lib.POLICY_MAX_ACTIONS, 'up to %d actions' % _lib.POLICY_MAX_ACTIONS
        single = np.ndim(v) == 1
        n = 1 if single else len(v)
        if k is None:
            # The stream hands out bounded draws (cobel_rng_bounded), not their words: the draw d
            # is made there, and the entry point is given the smallest word that maps to it.
            self._bind(n, device)
            d = torch.empty(n, dtype=torch.int32, device=device)
            _lib.check(_lib.lib().cobel_rng_bounded(
                _lib.ptr(self.counter), self.seed, self.stream, 0, A, _lib.ptr(d), n, 1, 1,
                _lib.current_stream(device)))
            k = ((d.to(torch.int64) << 32) + (A - 1)) // A
        else:
            k = torch.as_tensor(np.asarray(k, dtype=np.uint64).astype(np.int64), device=device)
        k = k.reshape(n).contiguous()
        act, _ = select_n(_lib.POLICY_RANDOM, None, None, None, k, None, n, A, device)
        return int(act[0].item()) if single else act

    def get_action_probs(self, v, mask=None):
        return np.full(self.actions, 1.0 / self.actions)
