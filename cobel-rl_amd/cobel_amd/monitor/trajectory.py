"""Trajectories of vectorised test runs.

The reference's ``TrajectoryMonitor`` (monitor/behavior.py:304-385) appends ``env.get_position()`` at
every ``on_step_end``.  Step hooks fire only with one instance here, so a test session of many
instances reports sums.  ``agent.rollout(env, trials, steps)`` is that session with a record: it
returns a ``TrajectoryRecord``, the states and actions of every instance, trial and step on the
device, which hands the monitor and ``get_occupancy_map`` what the step hook would have."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib


def record_bytes(n_envs: int, trials: int, steps: int) -> int:
    """Bytes of a record: int16 states and uint8 actions per step, int16 start and int32 length
    per trial."""
    return int(n_envs) * int(trials) * (3 * int(steps) + 6)


class TrajectoryRecord:
    """What each instance did in one ``rollout`` session.  For instance ``i``, session trial ``t``:

    * ``start   int16 [N, trials]``          the state after the reset,
    * ``states  int16 [N, trials, steps]``   the state entered by step ``k``,
    * ``actions uint8 [N, trials, steps]``   the action of step ``k``,
    * ``length  int32 [N, trials]``          the steps executed, ``logs['steps'] + 1``;

    entries at ``k >= length`` are ``-1`` (states) and ``255`` (actions).  ``interface`` is the
    environment of the session (the coordinates of its states), ``first_trial`` the agent's
    ``current_trial`` when the session began."""

    def __init__(self, interface, n_envs: int, trials: int, steps: int, device=None,
                 first_trial: int = 0) -> None:
        self.interface = interface
        self.n_envs, self.trials, self.steps = int(n_envs), int(trials), int(steps)
        assert self.n_envs >= 1 and self.trials >= 1 and self.steps >= 1, \
            'a record needs at least one instance, trial and step'
        self.first_trial = int(first_trial)
        self.instance_base = int(getattr(interface, 'instance_base', 0))
        self.device = torch.device(device if device is not None else interface.device)
        need = record_bytes(self.n_envs, self.trials, self.steps)
        if self.device.type == 'cuda':
            free = torch.cuda.mem_get_info(self.device)[0]
            if need > free:
                raise MemoryError(
                    'TrajectoryRecord: the record of %d instances, %d trials and %d steps takes '
                    '%d bytes (%.1f GiB), %d bytes of device memory are free'
                    % (self.n_envs, self.trials, self.steps, need, need / 2.0 ** 30, free))
        shape = (self.n_envs, self.trials)
        self.start = torch.full(shape, -1, dtype=torch.int16, device=self.device)
        self.length = torch.zeros(shape, dtype=torch.int32, device=self.device)
        # (the launch fills these two with the padding before its kernel writes the entries)
        self.states = torch.empty(shape + (self.steps,), dtype=torch.int16, device=self.device)
        self.actions = torch.empty(shape + (self.steps,), dtype=torch.uint8, device=self.device)

    # -- coordinates ------------------------------------------------------------------------------
    def world_of(self, instance: int) -> int:
        """Index of the world instance ``instance`` lives in (stacks of worlds)."""
        return (self.instance_base + int(instance)) % self._n_worlds()

    def _n_worlds(self) -> int:
        handle = getattr(self.interface, 'handle', None)
        if handle is not None:
            return int(handle.n_worlds)
        return len(getattr(self.interface, '_coords', [None]))

    def _positions(self, instance: int, states: np.ndarray) -> list:
        """What ``get_position()`` returns in each of ``states``: a gridworld's coordinates, a
        topology's whole pose."""
        env = self.interface
        if hasattr(env, '_coords'):
            table = env._coords[self.world_of(instance) % len(env._coords)]
        else:
            table = env.pose
        return [np.copy(table[int(s)]) for s in states]

    def trajectory(self, instance: int = 0, trial: int = 0) -> list:
        """The positions ``env.get_position()`` would have returned at each ``on_step_end`` of
        session trial ``trial`` of ``instance``: the states entered, without the start — the list
        the reference's ``TrajectoryMonitor`` appends for a trial."""
        n = int(self.length[instance, trial].item())
        states = self.states[instance, trial, :n].cpu().numpy()
        return self._positions(instance, states)

    def trajectories(self, instances=None) -> list:
        """``trajectory(i, t)`` of every trial of ``instances`` (all of them when None), in
        instance-major order; one copy of the record to the host."""
        chosen = range(self.n_envs) if instances is None else [int(i) for i in instances]
        length = self.length.cpu().numpy()
        states = self.states.cpu().numpy()
        return [self._positions(i, states[i, t, :length[i, t]])
                for i in chosen for t in range(self.trials)]

    # -- visit counts -------------------------------------------------------------------------------
    def visit_counts(self):
        """``int64 [n_worlds, S]``: how often each state was entered, computed on the device from
        ``states`` — the growth of ``agent.monitors.occupancy`` over the session, and what
        ``analysis.occupancy_from_counts`` takes."""
        handle = self.interface.handle
        counts = torch.zeros((handle.n_worlds, handle.n_states), dtype=torch.int64,
                             device=self.device)
        _lib.check(_lib.lib().cobel_rollout_visits(
            _lib.ptr(self.states), self.n_envs, self.trials * self.steps, handle.n_states,
            handle.n_worlds, self.instance_base, _lib.ptr(counts),
            _lib.current_stream(self.device)))
        return counts
