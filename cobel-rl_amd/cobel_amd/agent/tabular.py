"""Shared implementation of the two tabular TD agents on ``cobel_tab_run``."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..memory import _device
from ..policy.greedy import EpsilonGreedy, ExclusiveEpsilonGreedy
from ..policy.random import RandomDiscrete
from ..policy.softmax import Softmax
from .agent import FusedAgent

# the policies cobel_tab_policy_run selects with, and where each keeps its parameter
_POLICY_KINDS = {Softmax: (_lib.POLICY_SOFTMAX, 'beta'),
                 ExclusiveEpsilonGreedy: (_lib.POLICY_EXCLUSIVE, 'epsilon'),
                 RandomDiscrete: (_lib.POLICY_RANDOM, None)}


class TabularAgent(FusedAgent):
    """Q table [N, S, A] float32 on device (A = 4 but for the general kernel) + launch plumbing
    for ``cobel_tab_run``: ``FusedAgent._fill_run`` plus the table, the kind and the flags."""

    agent_kind = _lib.AGENT_Q
    general_actions = True     # cobel_tab_run's general kernel takes any action count
    exclusive_policy = True    # (_launch's policy runs; SFMA, with a launcher of its own, says False)
    force_general = False      # True: always the general kernel (tests, A/B comparisons)
    extra_flags = 0            # COBEL_F_* testing switches ORed into every launch (F_NO_PWG, ...)

    def __init__(self, observation_space, action_space, policy, policy_test, learning_rate,
                 gamma, custom_callbacks) -> None:
        super().__init__(observation_space, action_space, policy, policy_test, custom_callbacks)
        self.learning_rate = learning_rate
        self.gamma = gamma
        self._q = None
        self._q_host = (np.zeros((self.n_states, self.n_actions), dtype=np.float32)
                        if self.n_states is not None else None)
        self._poses = None      # node poses when the observations are a Topology's (Box)
        self._ppol = (None,) * 5   # parameter sets of policy runs: key, sets, index, count, policy_params

    # -- tables -----------------------------------------------------------------------------
    def _alloc_tables(self) -> None:
        self._q = torch.zeros((self.n_envs, self.n_states, self.n_actions), dtype=torch.float32,
                              device=self.device)
        # planning / replay batches the kernels evaluated (cobel_tab_run_t.batches_done): a Dyna-Q
        # batch is drawn every learning step, but evaluated only if it can change a table
        self.batches_done = torch.zeros(1, dtype=torch.int64, device=self.device)
        # work area of a launch (cobel_tab_run_t.scratch: ticket and slice counters of the
        # persistent-workgroup Dyna-Q kernel), one per agent: agents that share a world handle may
        # be in flight together
        # (zeroed once: its abort word is only ever raised by a launch, see check_launches)
        self._scratch = torch.zeros(_lib.tab_scratch_bytes(self.n_envs) // 4, dtype=torch.int32,
                                    device=self.device)
        if self._q_host is not None:
            self._q.copy_(torch.as_tensor(self._q_host, device=self.device).expand_as(self._q))

    @property
    def Q(self):
        """``(S, 4)`` float32 NumPy snapshot for one instance (the reference's ``agent.Q``), the
        device tensor ``[N, S, 4]`` when vectorised.  Assigning broadcasts to all instances."""
        if self._q is None:
            return self._q_host
        return self._q[0].cpu().numpy() if self.n_envs == 1 else self._q

    @Q.setter
    def Q(self, value) -> None:
        if self._q is None:
            self._q_host = np.array(value, dtype=np.float32).reshape(self.n_states, self.n_actions)
        else:
            v = torch.as_tensor(np.asarray(value, dtype=np.float32) if not torch.is_tensor(value)
                                else value, device=self.device).to(torch.float32)
            self._q.copy_(v.expand_as(self._q) if v.dim() == 2 else v)

    def predict_on_batch(self, batch):
        """Q-values of a batch of observations, ``[len(batch), 4]`` (dyna_q.py:303-317)."""
        if self._poses is not None:
            idx = self._node_index(batch)
        else:
            idx = np.array(batch).astype(int)
        if self._q is None:
            return self._q_host[idx]
        if self.n_envs == 1:
            return self._q[0][torch.as_tensor(idx, device=self.device)].cpu().numpy()
        return self._q[:, torch.as_tensor(idx, device=self.device)]

    def _node_index(self, batch) -> np.ndarray:
        """Pose observations -> node indices (the reference keys Q by tuple(pose), q.py:154-155;
        an unseen pose is a KeyError there as well)."""
        if len(batch) and isinstance(batch[0], dict):     # agent/q.py:156-158
            batch = [np.concatenate([np.asarray(o, dtype=np.float64).flatten()
                                     for _, o in b.items()]) for b in batch]
        obs = np.asarray(batch, dtype=np.float64).reshape(-1, self._poses.shape[1])
        hit = (obs[:, None, :] == self._poses[None, :, :]).all(axis=2)
        if not hit.any(axis=1).all():
            raise KeyError(tuple(obs[~hit.any(axis=1)][0]))
        return hit.argmax(axis=1)

    # -- launch -----------------------------------------------------------------------------
    def _extra(self, run: _lib.TabRun) -> None:
        pass

    def _model_lr(self):
        return 0.9

    def _launch(self, interface, pol, flags, trials_target, steps, budget, batch,
                describe=None, record=None) -> None:
        """One launch (or, with ``describe``, its plan): an EpsilonGreedy run is a ``cobel_tab_run_t``
        for ``cobel_tab_run`` / ``cobel_tab_rollout``; the policies of ``_POLICY_KINDS`` take the same
        run struct inside a ``cobel_tab_policy_run_t`` to ``cobel_tab_policy_run``."""
        greedy = type(pol) is EpsilonGreedy
        if not greedy:
            if type(pol) not in _POLICY_KINDS:
                raise NotImplementedError(
                    '%s selects with EpsilonGreedy, Softmax, ExclusiveEpsilonGreedy or RandomDiscrete; '
                    'got %s' % (type(self).__name__, type(pol).__name__))
            if record is not None:
                raise NotImplementedError('rollout records sessions that select with EpsilonGreedy; '
                                          'got %s' % type(pol).__name__)
            kind, attr = _POLICY_KINDS[type(pol)]
            if kind == _lib.POLICY_RANDOM:
                assert pol.actions == self.n_actions, \
                    'RandomDiscrete(%d) on a world of %d actions' % (pol.actions, self.n_actions)
        lib, world = _lib.lib(), interface.handle.ptr
        call = _lib.TabRun() if greedy else _lib.TabPolicyRun()
        run = call if greedy else call.run
        self._fill_run(run, interface, flags, trials_target, steps, budget)
        run.q = _lib.ptr(self._q)
        run.batches_done = _lib.ptr(self.batches_done)
        run.agent = self.agent_kind
        run.flags = flags | self.extra_flags
        run.batch = batch
        if greedy:
            run.scratch, run.scratch_bytes = _lib.ptr(self._scratch), self._scratch.numel() * 4
            if self.force_general:
                run.flags |= _lib.F_TAB_GENERAL
            self._hyper(run, self.learning_rate, self.gamma, pol.epsilon, self._model_lr())
        else:
            call.policy = kind
            self._hyper_policy(call, pol, attr)
        self._extra(run)
        if describe is not None:
            plan = lib.cobel_tab_describe if greedy else lib.cobel_tab_policy_plan
            _lib.check(plan(world, C.byref(call), describe))
            return
        # (the entry point SURVEY.md section 8b names for this agent: cobel_tab_run with the kind checked)
        if not greedy:
            entry = lib.cobel_tab_policy_run
        elif record is not None:    # rollout(): the same run struct around a trajectory record
            call, entry = self._rollout_struct(run, record, world), lib.cobel_tab_rollout
        else:
            entry = lib.cobel_dynaq_run if self.agent_kind == _lib.AGENT_DYNAQ else lib.cobel_q_run
        # (`launch_events`: a pair of torch.cuda.Event recorded right around the library call —
        #  bench.py times the kernel without the host's preparation of its arguments)
        #  (a LIST that gets one pair appended per launch: a train() call may issue several)
        ev = getattr(self, 'launch_events', None)
        pair = None
        if ev is not None:
            pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            pair[0].record()
        _lib.check(entry(world, C.byref(call), _lib.current_stream(self.device)))
        if pair is not None:
            pair[1].record()
            ev.append(pair)

    # -- Softmax, ExclusiveEpsilonGreedy, RandomDiscrete ------------------------------------------------
    def _hyper_policy(self, prun: _lib.TabPolicyRun, pol, attr) -> None:
        """``_hyper`` for a policy run: the learning rate, the discount, the model's learning rate and
        the policy's ``beta`` / ``epsilon``, each a scalar or one value per instance.  With an array
        among them the distinct combinations become parameter sets (their epsilon tables unused)
        plus the column ``policy_params``, and every instance gets the index of its combination."""
        run = prun.run
        param = 0.0 if attr is None else getattr(pol, attr)
        vals = (self.learning_rate, self.gamma, param, self._model_lr())
        cols = _device.param_columns(vals, self.n_envs)
        if cols is None:
            run.alpha, run.gamma, run.model_lr = float(vals[0]), float(vals[1]), float(vals[3])
            prun.policy_param = float(param)
            return

        def fill(rows):
            sets = (_lib.ParamSet * len(rows))()
            for k, (a, g, _, m) in enumerate(rows):
                _lib.check(_lib.lib().cobel_param_set_fill(float(a), float(g), 0.0, float(m),
                                                           C.byref(sets[k])))
            self._ppar_rows = np.ascontiguousarray(rows[:, 2], dtype=np.float64)
            return sets
        # (sets of their own, apart from the ones an EpsilonGreedy launch of this agent builds)
        new = _device.param_sets(cols, self._ppol[0], fill, self.device)
        if new is not None:
            self._ppol = new[:4] + (torch.as_tensor(self._ppar_rows, device=self.device),)
        _, sets_dev, index_dev, n_sets, ppar_dev = self._ppol
        run.alpha, run.gamma, run.model_lr = (float(v) for v in cols[0, [0, 1, 3]])
        prun.policy_param = float(cols[0, 2])
        run.param_sets, run.param_index = _lib.ptr(sets_dev), _lib.ptr(index_dev)
        run.n_param_sets = n_sets
        prun.policy_params = _lib.ptr(ppar_dev)

    # -- a test session that records ----------------------------------------------------------------
    rollout_element_stores = False   # True: one store per record entry (tests, A/B comparisons)

    def _rollout_struct(self, run: _lib.TabRun, record, world) -> _lib.TabRollout:
        ro = _lib.TabRollout()
        ro.run = run
        ro.start, ro.states = _lib.ptr(record.start), _lib.ptr(record.states)
        ro.actions, ro.length = _lib.ptr(record.actions), _lib.ptr(record.length)
        ro.trials, ro.steps = record.trials, record.steps
        ro.record_flags = _lib.ROLLOUT_ELEMENT_STORES if self.rollout_element_stores else 0
        out = (C.c_int32 * 4)()
        _lib.check(_lib.lib().cobel_tab_rollout_plan(world, C.byref(ro), out))
        self.rollout_plan = {'lds_bytes': int(out[0]), 'threads_per_workgroup': int(out[1]),
                             'instances_per_workgroup': int(out[2]), 'workgroups': int(out[3])}
        return ro

    def rollout(self, interface, trials: int, steps: int):
        """``test(interface, trials, steps)`` that also returns what every instance did, as a
        ``monitor.TrajectoryRecord`` on the device: the same draws, monitors, counters and final
        state, one launch (``cobel_tab_rollout``) whatever the instance count, ``Q`` untouched.
        Trial callbacks fire as in a vectorised session — ``on_trial_begin`` for every trial before
        the launch, ``on_trial_end`` after it with the means over instances; step callbacks do not
        fire: the record holds what they would have seen (``record.trajectory(i, t)``,
        ``TrajectoryMonitor.update_from_device(record)``)."""
        from ..monitor.trajectory import TrajectoryRecord
        trials, steps = int(trials), int(steps)
        if hasattr(interface, 'seq'):
            raise NotImplementedError('rollout records sessions on a Gridworld or a Topology')
        if trials < 1 or steps < 1:
            raise IndexError('rollout: trials = %d, steps = %d (both at least 1)' % (trials, steps))
        if type(self.policy_test) is not EpsilonGreedy:
            raise NotImplementedError('rollout records sessions that select with EpsilonGreedy; '
                                      'policy_test is a %s' % type(self.policy_test).__name__)
        pol, flags, first = self._session_begin(interface, trials, False)
        record = TrajectoryRecord(interface, self.n_envs, trials, steps, self.device, first)
        self._one_launch_session(first, trials, lambda: self._launch(
            interface, pol, flags, first + trials, steps, 0, 0, record=record))
        self._session_end(pol, interface)
        return record

    def check_launches(self) -> None:
        """Waits for this agent's launches and raises ``CobelHipError`` if a sliced launch of the
        persistent-workgroup kernel gave up waiting for a ring entry (``cobel_tab_scratch_check``:
        a lost producer wavefront ends in an error, not in a hung GPU)."""
        scratch = getattr(self, '_scratch', None)     # (SR / SFMA keep their own tables: no slices)
        if scratch is not None:
            _lib.check(_lib.lib().cobel_tab_scratch_check(
                _lib.ptr(scratch), scratch.numel() * 4, _lib.current_stream(self.device)))

    def env_steps(self) -> int:
        self.check_launches()
        return super().env_steps()

    def describe_launch(self, interface, pol, flags, trials_target, steps, budget, batch) -> dict:
        """Which kernel ``_launch`` would take with these arguments (``cobel_tab_describe``); for
        a Softmax, ExclusiveEpsilonGreedy or RandomDiscrete policy the plan of
        ``cobel_tab_policy_run`` (``cobel_tab_policy_plan``)."""
        out = (C.c_int32 * 4)()
        TabularAgent._launch(self, interface, pol, flags, trials_target, steps, budget, batch,
                             describe=out)
        if type(pol) is not EpsilonGreedy:
            return {'kernel': 'policy', 'lds_bytes': int(out[0]), 'threads_per_workgroup': int(out[1]),
                    'instances_per_workgroup': int(out[2]), 'workgroups': int(out[3])}
        return {'kernel': int(out[0]), 'lds_bytes': int(out[1]), 'workgroups_per_cu': int(out[2]),
                'instances_per_workgroup': int(out[3])}
