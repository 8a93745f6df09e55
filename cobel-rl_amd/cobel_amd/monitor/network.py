"""``cobel.monitor.RepresentationMonitor`` (monitor/network.py:15-126): the activity of one network
layer on a fixed set of observations, recorded over training.  Where the agent trains one network
per instance, the record holds every instance's activity."""
from __future__ import annotations

import numpy as np

from .behavior import Monitor


class RepresentationMonitor(Monitor):
    """Tracks the activity of layer ``layer`` of the agent's network ``model`` (an attribute name,
    e.g. ``'model_online'``) for ``observations``.  ``interval``: an int records every
    ``interval``-th call of ``update`` (0: every call), a tuple records at those trials.

    A record is the network's ``get_layer_activity`` result ``[U, P]``.  If the named network is
    the single copy of a stack of per-instance networks and the agent runs more than one instance,
    the record is the stack's ``[N, U, P]`` and the trace ``[T, N, U, P]``."""

    def __init__(self, model: str, layer, observations, interval=0, widget=None) -> None:
        super().__init__(widget)
        self.last_update = 1
        if type(interval) is int:
            assert interval >= 0
            self.last_update += interval
        elif type(interval) is tuple:
            assert min(interval) >= 0
        self.interval = interval
        self.layer = layer
        self.model = model
        self.observations = observations
        self.activity_trace: list = []

    def clear_plots(self) -> None:
        pass

    def _network(self, agent):
        """The stack behind the named network where the agent trains one network per instance,
        else the named network itself."""
        single = getattr(agent, self.model)
        n_envs = getattr(agent, 'n_envs', None)
        if n_envs is not None and n_envs > 1 and hasattr(agent, '_stacks'):
            for stack, net, instance in agent._stacks():
                if net is single and instance == 0 and stack is not None and \
                        getattr(stack, 'n', None) == n_envs:
                    return stack
        return single

    def update(self, logs) -> None:
        record = False
        if type(self.interval) is int:
            record = self.last_update >= self.interval
            self.last_update = 0
        elif type(self.interval) is tuple:
            record = logs['trial'] in self.interval
        if record:
            assert hasattr(logs['agent'], self.model)
            self.activity_trace.append(
                self._network(logs['agent']).get_layer_activity(self.observations, self.layer))
        self.last_update += 1

    def get_trace(self):
        return np.array(self.activity_trace)
