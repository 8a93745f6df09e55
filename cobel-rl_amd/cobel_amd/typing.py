"""Type aliases under the reference's names (``cobel.typing``), so that annotated user scripts
import unchanged.  Only the names the accelerated path's demos and tests use."""
from __future__ import annotations

from typing import Any, Callable, TypedDict

import numpy as np

NodeID = str
Pose = tuple
Node = dict            # {'pose', 'reward', 'terminal', 'neighbors'} (interface/topology.py:21-26)
Observation = Any      # int (gridworld state), numpy array (pose) or a dict of arrays
Action = Any
Logs = dict
Callback = Callable[[dict], Any]
CallbackDict = dict    # {'on_trial_begin' | 'on_step_begin' | 'on_step_end' | 'on_trial_end' | ...: [callables]}
NDArray = np.ndarray


class TrialStep(TypedDict):
    """One step of a predefined trial (interface/sequence.py:16-19): the name of its observation,
    its reward — one float, or an array indexed by the action — and an action that may overwrite
    the agent's."""
    observation: str
    reward: Any            # float | NDArray
    action: Any            # None | int


Trial = list               # list[TrialStep] (interface/sequence.py:22)
