"""Scalar policies — ``cobel.policy.scalar`` (policy/scalar.py:13-300): ``Proportional``,
``Threshold`` and ``Sigmoid`` turn one value into a binary action.

Constructors, assertions and attributes are the reference's (``Threshold.window`` is stored
halved), and ``get_action_probs`` evaluates the reference's expressions.  Like ``EpsilonGreedy`` the
classes carry parameters: the selection happens inside the kernel of the Rescorla-Wagner agents
(csrc/rw.hip) with the policy's Philox stream — one double draw per ``rng.random()``, one bounded
draw per ``rng.integers(2)``; ``Threshold`` draws only inside its window, so the draw counters of
the instances drift apart and the kernel carries one per instance.  Each float parameter may also
be an array with one entry per environment instance (sweeps); ``code_reverse`` stays one bool.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from .policy import Policy


class ScalarPolicy(Policy):
    """What the kernel reads of a scalar policy: its kind and the parameter row
    (threshold, window / 2, scale, value_max)."""
    kind = _lib.RW_POLICY_NONE

    def _row(self) -> tuple:
        return (getattr(self, 'threshold', 0.0), getattr(self, 'window', 0.0),
                getattr(self, 'scale', 0.0), self.value_max)

    def parameter_rows(self, n_envs: int) -> np.ndarray:
        """``[1, 4]`` float64, or ``[n_envs, 4]`` where a parameter is given per instance."""
        vals = [np.asarray(v, dtype=np.float64) for v in self._row()]
        if all(v.ndim == 0 for v in vals):
            return np.array([[float(v) for v in vals]], dtype=np.float64)
        for v in vals:
            assert v.ndim == 0 or v.shape == (n_envs,), \
                'per-instance policy parameters need one entry per environment instance'
        return np.array(np.stack([np.broadcast_to(v, (n_envs,)) for v in vals], axis=1), order='C')

    def select_action(self, v, mask=None):
        raise NotImplementedError(
            '%s.select_action: the selection happens inside the kernel of the Rescorla-Wagner '
            'agents; there is no single-call form' % type(self).__name__)


class Proportional(ScalarPolicy):
    kind = _lib.RW_POLICY_PROPORTIONAL

    def __init__(self, value_max: float = 1.0, code_reverse: bool = True, rng=None) -> None:
        super().__init__(rng)
        self.value_max = value_max
        self.code_reverse = code_reverse

    def get_action_probs(self, v, mask=None):
        """policy/scalar.py:70-91."""
        probs = np.abs(np.array([1.0, 0.0]) - v / self.value_max)
        return np.flip(probs) if self.code_reverse else probs


class Threshold(ScalarPolicy):
    kind = _lib.RW_POLICY_THRESHOLD

    def __init__(self, threshold: float = 0.5, window: float = 0.0, value_max: float = 1.0,
                 code_reverse: bool = True, rng=None) -> None:
        super().__init__(rng)
        threshold_, window_ = np.asarray(threshold), np.asarray(window)
        assert np.all(threshold_ >= 0.0) and np.all(threshold_ <= 1), \
            'Threshold must lie within the interval (0, 1)!'
        assert np.all(threshold_ - window_ / 2 > 0.0) and np.all(threshold_ + window_ / 2 < 1.0), \
            'The window for random actions extends over the value range!'
        self.threshold = threshold
        self.window = window / 2
        self.value_max = value_max
        self.code_reverse = code_reverse

    def get_action_probs(self, v, mask=None):
        """policy/scalar.py:174-197."""
        v = v / self.value_max
        probs = np.zeros(2)
        probs[int(self.code_reverse) - int(v > self.threshold)] = 1.0
        if v > self.threshold - self.window and v < self.threshold + self.window:
            probs.fill(0.5)
        return probs


class Sigmoid(ScalarPolicy):
    kind = _lib.RW_POLICY_SIGMOID

    def __init__(self, threshold: float = 0.5, scale: float = 10.0, value_max: float = 1.0,
                 code_reverse: bool = True, rng=None) -> None:
        super().__init__(rng)
        assert np.all(np.asarray(threshold) >= 0.0) and np.all(np.asarray(threshold) <= 1), \
            'Threshold must lie within the interval (0, 1)!'
        assert np.all(np.asarray(scale) >= 0.0), \
            "The sigmoid's scaling factor must be non-negative!"
        self.threshold = threshold
        self.scale = scale
        self.value_max = value_max
        self.code_reverse = code_reverse

    def get_action_probs(self, v, mask=None):
        """policy/scalar.py:276-300."""
        probs = np.abs(np.array([1.0, 0.0])
                       - 1 / (1 + np.exp(-(v / self.value_max - self.threshold) * self.scale)))
        return np.flip(probs) if self.code_reverse else probs
