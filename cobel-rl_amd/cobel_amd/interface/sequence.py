"""Vectorised Sequence environment — ``cobel.interface.Sequence`` (interface/sequence.py:25-215): it
plays back predefined trials of observation, reward and an optional forced action.

``Sequence(trials, observations, observation_space, nb_actions=1, overwrite=False)`` as in the
reference (there is no widget), plus ``n_envs``, ``seed``, ``device`` and ``instance_base`` as
``Gridworld`` and ``Topology`` have them.  ``trials`` is one schedule (a list of ``Trial``) or a list
of schedules of the same number of trials; ``schedule_of`` gives every instance its schedule
(round-robin by default), ``instance_ids`` the instance number its random streams are drawn with
(``instance_base + i`` by default).

The schedules are compiled once (``compile_schedules``) into tables on the device: the observation
table ``[K + 1, D]`` (row 0 is the zero observation of ``zero_current()``), per schedule step the
row of its observation, its reward row with the flag "one float", its forced action (-1 for
``None``), and the trial offsets.  ``current_trial`` / ``current_step`` are per instance and live on
the device; they follow sequence.py:129-204: ``end_trial`` rises with the trial's last step, only
then ``current_trial`` advances, ``reset()`` rewinds ``current_step`` alone.  The position depends
on the schedule and the step caps only, never on the actions, so the host keeps a mirror of it and
raises the reference's ``IndexError`` BEFORE a launch that would read past the last trial.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..spaces import Box, Discrete
from .gridworld import _as_seed
from .interface import Interface


def compile_schedules(schedules: list, observations: dict, nb_actions: int, overwrite: bool) -> dict:
    """The host tables of a list of schedules (each a list of trials, each a list of TrialSteps)."""
    names = list(observations.keys())
    assert len(names) > 0, 'a Sequence needs at least one observation'
    first = np.asarray(observations[names[0]])
    rows = [np.zeros(first.size, dtype=np.float64)]
    for k in names:
        o = np.asarray(observations[k], dtype=np.float64)
        assert o.shape == first.shape, 'all observations of a Sequence have one shape'
        rows.append(o.reshape(-1))
    row_of = {k: i + 1 for i, k in enumerate(names)}
    n_trials = len(schedules[0])
    assert n_trials >= 1, 'a Sequence needs at least one trial'
    step_obs, step_action, step_scalar, step_reward, offsets = [], [], [], [], []
    for schedule in schedules:
        assert len(schedule) == n_trials, \
            'all schedules of a Sequence have the same number of trials (%d and %d)' % (
                n_trials, len(schedule))
        off = []
        for trial in schedule:
            assert len(trial) >= 1, 'a trial needs at least one step'
            off.append(len(step_obs))
            for st in trial:
                step_obs.append(row_of[st['observation']])     # (KeyError as in the reference)
                act = st.get('action')
                step_action.append(-1 if act is None else int(act))
                r = st['reward']
                if type(r) is float:                            # sequence.py:159
                    step_scalar.append(1)
                    step_reward.append([r] + [0.0] * (nb_actions - 1))
                else:
                    r = np.asarray(r, dtype=np.float64)
                    if r.shape != (nb_actions,):
                        raise ValueError('a reward is one float or an array with one entry per '
                                         'action (%d), not %r' % (nb_actions, st['reward']))
                    assert not overwrite or (act is not None and 0 <= int(act) < nb_actions), \
                        'overwrite=True: a step with an array reward needs its action'
                    step_scalar.append(0)
                    step_reward.append(list(r))
        off.append(len(step_obs))
        offsets.append(off)
    return dict(
        obs_table=np.ascontiguousarray(np.stack(rows)), shape=first.shape,
        step_obs=np.array(step_obs, dtype=np.int32), step_action=np.array(step_action, dtype=np.int32),
        step_scalar=np.array(step_scalar, dtype=np.uint8),
        step_reward=np.ascontiguousarray(np.array(step_reward, dtype=np.float64).reshape(-1, nb_actions)),
        trial_off=np.array(offsets, dtype=np.int32), names=names)


class Sequence(Interface):
    def __init__(self, trials: list, observations: dict, observation_space, nb_actions: int = 1,
                 overwrite: bool = False, n_envs: int = 1, seed: int | None = None, device=None,
                 schedule_of=None, instance_base: int = 0, instance_ids=None) -> None:
        super().__init__(None)
        self.trials = trials
        self.overwrite = overwrite
        self.observations = observations
        self.observation_space = observation_space
        self.action_space = Discrete(nb_actions)
        if type(observation_space) is not Box:
            raise NotImplementedError(
                'Sequence: %s observation spaces — this version serves Box observation spaces'
                % type(observation_space).__name__)
        dim = int(np.prod(np.asarray(next(iter(observations.values()))).shape))
        if not 1 <= dim <= _lib.RW_MAX_DIM:
            raise NotImplementedError(
                'Sequence: observations of %d components — this version serves Box observations of '
                '1 to %d components' % (dim, _lib.RW_MAX_DIM))
        assert int(nb_actions) >= 1
        several = len(trials) > 0 and len(trials[0]) > 0 and isinstance(trials[0][0], list)
        self.schedules = list(trials) if several else [trials]
        self.tables = compile_schedules(self.schedules, observations, int(nb_actions), bool(overwrite))
        self.dim, self.n_trials = dim, self.tables['trial_off'].shape[1] - 1
        self.has_array_rewards = bool((self.tables['step_scalar'] == 0).any())
        self.n_envs = int(n_envs)
        self.seed = _as_seed(None) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.instance_base = int(instance_base)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        N, dev, S = self.n_envs, self.device, len(self.schedules)
        if schedule_of is None:
            schedule_of = np.arange(N) % S
        self.schedule_of = np.asarray(schedule_of, dtype=np.int32).reshape(-1)
        assert self.schedule_of.shape == (N,) and (self.schedule_of >= 0).all() and \
            (self.schedule_of < S).all(), 'schedule_of: one schedule index per instance'
        self.instance_ids = None
        if instance_ids is not None:
            ids = np.asarray(instance_ids, dtype=np.int64).reshape(-1)
            assert ids.shape == (N,) and (ids >= 0).all() and (ids < 2**32).all(), \
                'instance_ids: one instance number per instance'
            self.instance_ids = torch.as_tensor(ids.astype(np.uint32).view(np.int32), device=dev)
        self._dev = {k: torch.as_tensor(self.tables[k], device=dev).contiguous()
                     for k in ('obs_table', 'step_obs', 'step_action', 'step_scalar', 'step_reward',
                               'trial_off')}
        self._dev['schedule_of'] = torch.as_tensor(self.schedule_of, device=dev)
        self._trial = torch.zeros(N, dtype=torch.int32, device=dev)
        self._step = torch.zeros(N, dtype=torch.int32, device=dev)
        self._obs = torch.zeros((N, dim), dtype=torch.float64, device=dev)
        self._reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self._end = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._info = torch.zeros((N, 2), dtype=torch.int32, device=dev)
        # the host's mirror of the position (see the module docstring)
        self._trial_len = np.diff(self.tables['trial_off'], axis=1)
        self._h_trial = np.zeros(N, dtype=np.int64)
        self._h_step = np.zeros(N, dtype=np.int64)
        seq = _lib.Seq()
        for k, t in self._dev.items():
            setattr(seq, k, _lib.ptr(t))
        seq.cur_trial, seq.cur_step = _lib.ptr(self._trial), _lib.ptr(self._step)
        seq.n, seq.dim, seq.n_obs, seq.n_actions = N, dim, self.tables['obs_table'].shape[0], int(nb_actions)
        seq.n_schedules, seq.n_trials = S, self.n_trials
        seq.n_steps, seq.overwrite = len(self.tables['step_obs']), int(bool(overwrite))
        self.seq = seq
        self.current_observation = None
        self.zero_current()

    # -- position -----------------------------------------------------------------------------
    @property
    def current_trial(self):
        return int(self._trial[0].item()) if self.n_envs == 1 else self._trial

    @property
    def current_step(self):
        return int(self._step[0].item()) if self.n_envs == 1 else self._step

    def _past_the_end(self, what: str, instance: int):
        return IndexError('list index out of range: %s of instance %d would read past the last of '
                          'the %d trials' % (what, instance, self.n_trials))

    def _walk(self, trials: int, steps: int):
        """``trials`` trials under the cap ``steps``, walked once per (schedule, trial) the
        instances stand in: per instance the trial it ends in, the step its last trial stopped at
        (-1 for a session of no trials) and the steps it takes.  ``IndexError`` if an instance
        would begin a trial past its last one."""
        keys = np.stack([self.schedule_of.astype(np.int64), self._h_trial], axis=1)
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        ends, stops, totals = (np.empty(len(uniq), dtype=np.int64) for _ in range(3))
        for u, (s, p) in enumerate(uniq):
            step, total = -1, 0
            for _ in range(int(trials)):
                if p >= self.n_trials:
                    raise self._past_the_end('a session of %d trials' % trials,
                                             int(np.flatnonzero(inv == u)[0]))
                length = int(self._trial_len[s, p])
                step = min(length, int(steps))
                total += step
                p += int(length <= steps)
            ends[u], stops[u], totals[u] = p, step, total
        return ends[inv], stops[inv], totals[inv]

    def plan_session(self, trials: int, steps: int):
        """Where every instance stands after ``trials`` trials under the cap ``steps``:
        (current_trial, current_step) as arrays.  ``IndexError`` if an instance would begin a
        trial past its last one."""
        trial, step, _ = self._walk(trials, steps)
        return trial, np.where(step < 0, self._h_step, step)

    def session_steps(self, trials: int, steps: int) -> np.ndarray:
        """Steps every instance takes in such a session: the schedule and the cap fix them."""
        return self._walk(trials, steps)[2]

    def commit_session(self, trials: int, steps: int) -> None:
        """The mirror follows a session the device has run."""
        self._h_trial, self._h_step = self.plan_session(trials, steps)

    def step_at(self, instance, step=0):
        """(index into the step tables, length of the trial) of step ``step`` of the trial
        ``instance`` stands in; ``instance`` is an index or whatever NumPy indexes with."""
        s, p = self.schedule_of[instance], self._h_trial[instance]
        return (self.tables['trial_off'][s, p] + step,
                self._trial_len[s, np.minimum(p, self.n_trials - 1)])

    def _on_device(self) -> None:
        if self.device.type != 'cuda':
            raise _lib.CobelHipError('this Sequence was built on the host (device=%s): step, reset '
                                     'and the agents need a GPU' % self.device)

    # -- reference surface ----------------------------------------------------------------------
    def zero_current(self) -> None:
        """sequence.py:115-127."""
        if self.n_envs == 1:
            self.current_observation = np.zeros(self.tables['shape'])
        else:
            self.current_observation = torch.zeros((self.n_envs,) + tuple(self.tables['shape']),
                                                   dtype=torch.float64, device=self.device)

    def _observation(self):
        if self.n_envs == 1:
            self.current_observation = self._obs[0].cpu().numpy().reshape(self.tables['shape'])
            return self.current_observation.copy()
        # (a fresh tensor, not a view of the buffer the next call overwrites)
        self.current_observation = self._obs.reshape((self.n_envs,) + tuple(self.tables['shape'])).clone()
        return self.current_observation

    def step(self, action):
        self._on_device()
        N, A = self.n_envs, int(self.action_space.n)
        at, length = self.step_at(slice(None), self._h_step)
        bad = (self._h_trial >= self.n_trials) | (self._h_step >= length)
        if bad.any():
            raise self._past_the_end('step()', int(np.flatnonzero(bad)[0]))
        # a step with an array reward indexes it with the action (sequence.py:165), unless it is
        # overwritten: out of range is the reference's IndexError, negative counts from the end
        indexed = (self.tables['step_scalar'][at] == 0) & (not self.overwrite)
        if N == 1 and not torch.is_tensor(action):
            act = torch.full((1,), int(action), dtype=torch.int32, device=self.device)
        else:
            act = torch.as_tensor(action, device=self.device).to(torch.int32).contiguous()
            assert act.shape == (N,), 'one action per instance'
        given = act      # (log['action'] is the action as given, sequence.py:156)
        if indexed.any():
            a = act.cpu().numpy().astype(np.int64)
            bad = indexed & ((a < -A) | (a >= A))
            if bad.any():
                raise IndexError('index %d is out of bounds for axis 0 with size %d (instance %d)'
                                 % (a[bad][0], A, int(np.flatnonzero(bad)[0])))
            wrap = indexed & (a < 0)
            if wrap.any():
                act = torch.as_tensor(np.where(wrap, a + A, a).astype(np.int32), device=self.device)
        _lib.check(_lib.lib().cobel_seq_step(
            C.byref(self.seq), _lib.ptr(act), _lib.ptr(self._obs), _lib.ptr(self._reward),
            _lib.ptr(self._end), _lib.ptr(self._info), _lib.current_stream(self.device)))
        self._h_step = self._h_step + 1
        self._h_trial = self._h_trial + (self._h_step >= length)
        obs = self._observation()
        if N == 1:
            end = bool(self._end[0].item())
            info = self._info[0].cpu().numpy()
            return obs, float(self._reward[0].item()), end, end, {
                'action': int(action), 'step_action': None if info[1] < 0 else int(info[1])}
        end = self._end.bool()
        return obs, self._reward.clone(), end, end, {'action': given.clone(),
                                                     'step_action': self._info[:, 1].clone()}

    def reset(self):
        self._on_device()
        bad = self._h_trial >= self.n_trials
        if bad.any():
            raise self._past_the_end('reset()', int(np.flatnonzero(bad)[0]))
        _lib.check(_lib.lib().cobel_seq_reset(C.byref(self.seq), _lib.ptr(self._obs),
                                              _lib.current_stream(self.device)))
        self._h_step = np.zeros(self.n_envs, dtype=np.int64)
        return self._observation(), {}

    def get_position(self):
        return np.array([])
