"""Memory module of the SFMA agent — ``cobel.memory.SFMAMemory`` (memory/sfma.py:19-416).

Same constructor, attributes and methods as the reference.  Inside ``SFMA.train`` the store and
the replay are folded into the fused kernel (``cobel_sfma_run``); called on the memory itself,
``store`` / ``replay`` / ``retrieve_random_batch`` are device calls on the same tables
(``cobel_sfma_store`` / ``cobel_sfma_replay`` / ``cobel_sfma_random_batch``, csrc/sfma_mem.hip:
the kernel code of the fused kernel), and ``replay_batch`` runs K independent replays of every
instance side by side.  A memory is bound to a device by the agent's first session or, without an
agent, by ``bind``.  The methods draw from the memory stream of the session (seed, instance base)
at ``counter``, where ``train`` left it and where ``train`` goes on afterwards.  ``bind``, the
per-instance argument checks and the decoding of the packed model table are memory/_device.py's,
shared with ``PMAMemory`` and ``DynaQMemory``; ``_fill_params`` serves the agent's launcher too.

Per-instance parameters.  ``decay_inhibition``, ``decay_strength``, ``learning_rate``, ``beta``,
``C_step``, ``I_step``, ``R_threshold``, ``reward_modulation``, ``blend``, ``interpolation_fwd``
and ``interpolation_rev`` take a scalar or one entry per instance, ``mode`` a string or a sequence
of N strings: a sweep over them rides on the instance axis of one launch
(``optimizer.grid_search.spread_over_instances``).  The switches and ``decay_recency`` are
launch-wide; an array there is a ``NotImplementedError``.

This class owns the parameters and the device tables:

  ``table``     packed model records [N, S, 4] (float32 reward estimate, next state, nonterminal),
                decoded by ``rewards`` / ``states`` / ``terminals``
  ``strength``  experience strengths ``C`` float64 [N, 4S], experience index a * S + s
  ``stamp``     store clock of each experience; ``T`` is derived from it (the reference rescales the
                whole recency vector on every store: T[j] = decay_recency ** age, by repeated
                multiplication, 0 after the end-of-trial reset)
  ``state``     per-instance words: clock, epoch, replay mode, |TD| sum, agent-stream counter
``I`` (inhibition) only lives inside a replay; the one a host-called ``replay`` leaves is kept.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import _device

EXPERIENCE = np.dtype([('state', '<i4'), ('action', '<i4'), ('next_state', '<i4'),
                       ('nonterminal', '<i4'), ('reward', '<f8'), ('td', '<f8')])
EVENT = np.dtype([('sa', '<u4'), ('next', '<u4'), ('reward', '<f4'), ('trial', '<i4'),
                  ('td', '<f8')])
# the attributes that take a scalar or one entry per instance, in the order of the ten doubles of
# a cobel_sfma_param_set_t (_lib.SFMA_SET_MEMORY); `learning_rate` is the set's model_lr
SET_ATTRIBUTES = ('decay_inhibition', 'decay_strength', 'C_step', 'I_step', 'R_threshold', 'beta',
                  'reward_modulation', 'blend', 'interpolation_fwd', 'interpolation_rev')
# launch-wide: they change the code path (the switches) or the shape of the launch
LAUNCH_WIDE = ('deterministic', 'recency', 'C_normalize', 'D_normalize', 'R_normalize',
               'reward_mod_local', 'reward_mod', 'state_mod', 'error_mod_local', 'error_mod',
               'decay_recency')


def refuse_arrays(obj, names) -> None:
    """An array where one value serves the whole launch is refused, naming the attribute."""
    for name in names:
        if np.ndim(getattr(obj, name)) > 0:
            raise NotImplementedError(
                '%s.%s is launch-wide: one value for all instances, not an array'
                % (type(obj).__name__, name))


class SFMAMemory(_device.DeviceMemory, _device.PackedModel):
    def __init__(self, metric, nb_states: int, nb_actions: int, decay_inhibition: float = 0.9,
                 decay_strength: float = 1.0, learning_rate: float = 0.9, rng=None) -> None:
        assert nb_actions == 4, 'the model record layout covers 4-action worlds'
        self.rng = rng
        self.nb_states, self.nb_actions = nb_states, nb_actions
        self.decay_inhibition, self.decay_strength = decay_inhibition, decay_strength
        self.decay_recency = 0.9
        self.learning_rate = learning_rate
        self.beta = 20
        self.rlAgent = None
        self.reward_mod_local = self.error_mod_local = False
        self.reward_mod = self.error_mod = False
        self.policy_mod = self.state_mod = False
        self.metric = metric
        self.C_step = self.I_step = 1.0
        self.R_threshold = 10.0 ** -6
        self.deterministic = self.recency = False
        self.C_normalize = self.D_normalize = False
        self.R_normalize = True
        self.mode = 'default'
        self.reward_modulation = 1.0
        self.blend = 0.1
        self.interpolation_fwd, self.interpolation_rev = 0.5, 0.5
        self.table = self.strength = self.stamp = self.state = self.counter = None
        self._metric_dev = self._metric_src = self._metric_version = None
        self._recency = None
        # the session the host-called methods draw in: seed, instance base, worlds of the metric
        self.seed, self.instance_base, self._n_worlds = 0, 0, 1
        self.launch_flags = 0      # testing: _lib.F_SFMA_STREAM / F_FORCE_WAVE / F_NO_PREFETCH
        self._inhibition = None
        self._psets = {}           # parameter sets on the device, per caller: key, sets, index, n

    # -- device state ---------------------------------------------------------------------------
    def _bind(self, n_envs: int, device) -> None:
        if self.table is not None:
            return
        S = self.nb_states
        self.table = torch.empty((n_envs, S, 4), dtype=torch.int64, device=device)
        _lib.check(_lib.lib().cobel_model_init(_lib.ptr(self.table), n_envs, S,
                                               _lib.current_stream(device)))
        self.strength = torch.zeros((n_envs, 4 * S), dtype=torch.float64, device=device)
        self.stamp = torch.zeros((n_envs, 4 * S), dtype=torch.int32, device=device)
        self.state = torch.zeros((n_envs, _lib.SI_WORDS), dtype=torch.int32, device=device)
        self.state[:, _lib.SI_FLAGS] = 1       # agent.td starts as a weak Python float
        self._write_mode()
        self.counter = torch.zeros(n_envs, dtype=torch.int32, device=device)

    def _metric_on(self, device, n_worlds: int):
        """metric.D on the device, [n_worlds, S, S]: one matrix shared by all worlds, or a stack.
        A float64 contiguous tensor on ``device`` (a metric with ``compute='device'``) is used where
        it lies, without a copy: what ``update_transitions()`` writes into it in stream order is
        what the next launch reads.  One [S, S] matrix for several worlds is expanded into a stack of
        the memory's own, again after each ``update_transitions()`` of the metric."""
        src = self.metric.D if hasattr(self.metric, 'D') else self.metric
        S, dev = self.nb_states, torch.device(device)
        version = getattr(self.metric, 'version', None)     # (device metrics count their updates)
        if isinstance(src, torch.Tensor) and src.is_cuda and dev.type == 'cuda' \
                and dev.index in (None, src.device.index):
            assert src.dtype == torch.float64 and src.is_contiguous(), \
                'a device metric is a contiguous float64 tensor'
            if src.dim() == 3 or n_worlds == 1:
                assert tuple(src.shape) in ((S, S), (n_worlds, S, S)), \
                    'metric.D must be [S, S] or [n_worlds, S, S]'
                return src
            assert tuple(src.shape) == (S, S), 'metric.D must be [S, S] or [n_worlds, S, S]'
            if self._metric_dev is None or self._metric_src is not src \
                    or self._metric_version != version:
                if self._metric_dev is None or self._metric_src is not src:
                    self._metric_dev = torch.empty((n_worlds, S, S), dtype=torch.float64,
                                                   device=src.device)
                self._metric_dev.copy_(src.expand(n_worlds, S, S))
                self._metric_src, self._metric_version = src, version
            return self._metric_dev
        if self._metric_dev is None or self._metric_src is not src:
            D = np.asarray(src.cpu().numpy() if isinstance(src, torch.Tensor) else src,
                           dtype=np.float64)
            if D.ndim == 2:
                D3 = np.broadcast_to(D, (n_worlds, S, S))
            else:
                D3 = D
            assert D3.shape == (n_worlds, S, S), 'metric.D must be [S, S] or [n_worlds, S, S]'
            self._metric_dev = torch.as_tensor(np.array(D3, dtype=np.float64, order='C'), device=device)
            self._metric_src = src
        return self._metric_dev

    def _recency_table(self, device):
        """1, d, fl(d d), ...: what ``T *= decay_recency`` leaves after k stores."""
        if self._recency is None or self._recency[0] != self.decay_recency:
            vals, v = [1.0], 1.0
            while len(vals) < 16384:
                nv = v * self.decay_recency
                if nv == v:
                    break
                vals.append(nv)
                v = nv
            self._recency = (self.decay_recency,
                             torch.as_tensor(np.array(vals, dtype=np.float64), device=device))
        return self._recency[1]

    def _mode_key(self):
        """``mode`` as a string (all instances) or a tuple of N strings (one per instance)."""
        return self.mode if isinstance(self.mode, str) else tuple(str(m) for m in self.mode)

    def _mode_id(self):
        # memory/sfma.py:289-307 is an if/elif chain over the known names: any other string
        # (unit_tests/test_sfma.py assigns 'dynamic') leaves the similarity as in 'default'
        ident = lambda m: _lib.SFMA_MODES.index(m) if m in _lib.SFMA_MODES else 0   # noqa: E731
        key = self._mode_key()
        return ident(key) if isinstance(key, str) else [ident(m) for m in key]

    def _write_mode(self) -> None:
        ids = self._mode_id()
        if isinstance(ids, list):
            assert len(ids) == self.state.shape[0], _device.PER_INSTANCE_SHAPE
            ids = torch.as_tensor(ids, dtype=torch.int32, device=self.state.device)
        self.state[:, _lib.SI_MODE] = ids
        self._mode_seen = self._mode_key()

    def _sync_mode(self) -> None:
        if self._mode_key() != self._mode_seen:
            self._write_mode()

    def _read_mode(self) -> None:
        if self.state.shape[0] == 1:
            self.mode = self._mode_seen = _lib.SFMA_MODES[int(self.state[0, _lib.SI_MODE])]

    # -- the reference's tables -----------------------------------------------------------------
    @property
    def C(self):
        return self._squeeze(self.strength.cpu().numpy())

    @C.setter
    def C(self, value) -> None:
        self.strength.copy_(torch.as_tensor(np.asarray(value, dtype=np.float64),
                                            device=self.strength.device).expand_as(self.strength))

    @property
    def T(self):
        tab = self._recency_table(self.stamp.device).cpu().numpy()
        st = self.stamp.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        w = self.state.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        clock, epoch = w[:, _lib.SI_CLOCK:_lib.SI_CLOCK + 1], w[:, _lib.SI_EPOCH:_lib.SI_EPOCH + 1]
        age = np.minimum(clock - st, len(tab) - 1)
        return self._squeeze(np.where(st > epoch, tab[np.maximum(age, 0)], 0.0))

    @property
    def I(self):  # noqa: E743
        """The inhibition the last host-called ``replay`` left (of replay 0 for ``replay_batch``);
        zeros before the first one."""
        if self._inhibition is None:
            n = 1 if self.table is None else self.table.shape[0]
            return self._squeeze(np.zeros((n, self.nb_states)))
        return self._squeeze(self._inhibition)

    @property
    def modes(self):
        """Replay mode of every instance (they differ in dynamic mode)."""
        return [_lib.SFMA_MODES[int(m)] for m in self.state[:, _lib.SI_MODE].cpu().numpy()]

    def retrieve(self, state: int, action: int) -> dict:
        r, s, t = self._decode()
        return {'state': state, 'action': action, 'reward': r[0, state, action],
                'next_state': s[0, state, action], 'terminal': t[0, state, action]}

    # -- the reference's methods as device calls (csrc/sfma_mem.hip) ------------------------------
    def _fill_params(self, struct, agent=None) -> int:
        """The recency table, ``model_lr`` and the ten doubles of a ``cobel_sfma_run_t`` or
        ``cobel_sfma_mem_t`` — and, for the agent's launcher, ``agent = (learning rate, gamma,
        epsilon)`` — as scalars, or, if any of them has one entry per instance, as parameter sets:
        the distinct rows become ``cobel_sfma_param_set_t`` records, every instance gets the index
        of its row, and the scalar fields hold set 0's values as placeholders.  Returns the
        memory's ``SF_*`` switches (the caller ORs in its own)."""
        refuse_arrays(self, LAUNCH_WIDE)
        sf = 0
        for flag, on in ((_lib.SF_DETERMINISTIC, self.deterministic), (_lib.SF_RECENCY, self.recency),
                         (_lib.SF_C_NORMALIZE, self.C_normalize),
                         (_lib.SF_D_NORMALIZE, self.D_normalize),
                         (_lib.SF_R_NORMALIZE, self.R_normalize),
                         (_lib.SF_REWARD_MOD_LOCAL, self.reward_mod_local),
                         (_lib.SF_REWARD_MOD, self.reward_mod), (_lib.SF_STATE_MOD, self.state_mod)):
            sf |= flag if on else 0
        if self.recency:
            tab = self._recency_table(self.table.device)
            struct.recency_tab, struct.recency_len = _lib.ptr(tab), tab.numel()
        names = (('alpha', 'gamma', 'epsilon') if agent is not None else ()) + \
            ('model_lr',) + _lib.SFMA_SET_MEMORY
        vals = (tuple(agent) if agent is not None else ()) + (self.learning_rate,) + \
            tuple(getattr(self, a) for a in SET_ATTRIBUTES)
        n = self.table.shape[0]
        cols = _device.param_columns(vals, n)
        if cols is None:
            for name, v in zip(names, vals):
                setattr(struct, name, float(v))
            return sf
        if agent is None:          # the memory's own calls: the agent part at its defaults
            cols = np.concatenate([np.broadcast_to([0.99, 0.99, 0.0], (n, 3)), cols], axis=1)

        def fill(rows):
            sets = (_lib.SFMAParamSet * len(rows))()
            for k, row in enumerate(rows):
                _lib.check(_lib.lib().cobel_sfma_param_set_fill(
                    float(row[0]), float(row[1]), float(row[2]), float(row[3]),
                    C.byref((C.c_double * 10)(*row[4:])), C.byref(sets[k])))
            return sets
        who = 'agent' if agent is not None else 'memory'
        held = self._psets.setdefault(who, dict(key=None, sets=None, index=None, n=0, first=None))
        new = _device.param_sets(cols, held['key'], fill, self.table.device)
        if new is not None:
            held['key'], held['sets'], held['index'], held['n'], held['first'] = new
        for name, v in zip(names, held['first'][-len(names):]):   # placeholders: set 0's values
            setattr(struct, name, float(v))
        struct.param_sets, struct.param_index = _lib.ptr(held['sets']), _lib.ptr(held['index'])
        struct.n_param_sets = held['n']
        return sf

    def _mem(self, mem_flags: int = 0):
        assert self._is_bound, _device.NOT_BOUND
        dev = self.table.device
        m = _lib.SFMAMem()
        m.model, m.strength, m.stamp = _lib.ptr(self.table), _lib.ptr(self.strength), _lib.ptr(self.stamp)
        m.sfma_inst, m.counter = _lib.ptr(self.state), _lib.ptr(self.counter)
        m.metric = _lib.ptr(self._metric_on(dev, self._n_worlds))
        m.n, m.n_states, m.n_worlds = self.table.shape[0], self.nb_states, self._n_worlds
        m.instance_base = self.instance_base
        m.flags, m.sfma_flags, m.mem_flags = self.launch_flags, self._fill_params(m), mem_flags
        m.seed = self.seed
        self._sync_mode()
        return m, dev

    def launch_plan(self):
        """(form, LDS bytes, threads per workgroup, streaming tier) of the memory's launches."""
        return list(_device.plan4(_lib.lib().cobel_sfma_mem_plan, self.nb_states,
                                  self.launch_flags))

    def _per_instance(self, value, name: str, limit: int):
        """None / scalar / [N] -> None / int32 [N], range-checked."""
        return _device.per_instance(value, self.table.shape[0], name, limit)

    def store(self, experience: dict) -> None:
        """memory/sfma.py:195-236.  One experience per instance: with several instances the values
        of ``experience`` are scalars (the same for all) or [N] arrays.  ``'terminal'`` holds what
        the reference's agent puts there, 1 - end_trial.  ``'td'`` is read under ``error_mod`` /
        ``error_mod_local`` only (KeyError without it, as in the reference)."""
        refuse_arrays(self, LAUNCH_WIDE)
        flags = (_lib.SFM_ERROR_MOD_LOCAL if self.error_mod_local else 0) | \
                (_lib.SFM_ERROR_MOD if self.error_mod else 0)
        m, dev = self._mem(flags)
        S = self.nb_states
        rec = _device.records(experience, m.n, EXPERIENCE,
                              {'state': S, 'action': self.nb_actions, 'next_state': S},
                              skip=() if flags else ('td',))
        exps = torch.as_tensor(rec.view(np.uint8), device=dev)
        _lib.check(_lib.lib().cobel_sfma_store(C.byref(m), _lib.ptr(exps), _lib.current_stream(dev)))

    def _replay(self, n_replays: int, length: int, state, action, strided: bool):
        m, dev = self._mem(_lib.SFM_STRIDED if strided else 0)
        n, S = m.n, self.nb_states
        assert n_replays >= 1 and length >= 0
        st = self._per_instance(state, 'current_state', S)
        ac = self._per_instance(action, 'current_action', self.nb_actions)
        if st is None and bool((self.strength.clamp(min=0).sum(dim=1) == 0).any()):
            # P = clip(C) / sum(clip(C)) is 0 / 0: Generator.choice refuses NaN probabilities
            raise ValueError('probabilities contain NaN')
        st_d = None if st is None else torch.as_tensor(st, device=dev)
        ac_d = None if ac is None else torch.as_tensor(ac, device=dev)
        events = torch.zeros((n, n_replays, max(length, 1) * _lib.SFMA_EVENT_BYTES),
                             dtype=torch.uint8, device=dev)
        lengths = torch.zeros((n, n_replays), dtype=torch.int32, device=dev)
        inhibition = torch.zeros((n, S), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().cobel_sfma_replay(
            C.byref(m), n_replays, length, _lib.ptr(st_d), _lib.ptr(ac_d), _lib.ptr(events),
            _lib.ptr(lengths), _lib.ptr(inhibition), _lib.current_stream(dev)))
        self._inhibition = inhibition.cpu().numpy()
        ev = events.cpu().numpy().view(EVENT).reshape(n, n_replays, max(length, 1))[:, :, :length]
        return ev, lengths.cpu().numpy()

    @staticmethod
    def _experiences(ev) -> list:
        """Event records -> the reference's experience dicts (reward: the float32 table entry)."""
        sa = ev['sa'].astype(np.int64)
        return [{'state': int(s & 0xFFFF), 'action': int((s >> 16) & 0xFF), 'reward': r,
                 'next_state': int(ns), 'terminal': int((s >> 24) & 1)}
                for s, r, ns in zip(sa, ev['reward'], ev['next'])]

    def replay(self, replay_length: int, current_state=None, current_action=None) -> list:
        """memory/sfma.py:238-347: one replay per instance, drawing what the reference draws.  A
        list of experience dicts; one such list per instance when there are several (``current_*``
        are then scalars or [N] arrays)."""
        ev, lens = self._replay(1, replay_length, current_state, current_action, False)
        out = [self._experiences(ev[i, 0, :lens[i, 0]]) for i in range(ev.shape[0])]
        return out[0] if len(out) == 1 else out

    def replay_batch(self, n_replays: int, replay_length: int, current_state=None,
                     current_action=None) -> dict:
        """``n_replays`` independent replays of every instance from the memory as it stands, side by
        side on the device.  Replay k draws from index ``counter + k * (replay_length + 2)`` of the
        memory stream; the counter advances by ``n_replays * (replay_length + 2)``.  Arrays
        ``state`` / ``action`` / ``reward`` / ``next_state`` / ``terminal`` [N, K, L] (valid up to
        ``length`` [N, K]; -1 / NaN behind it)."""
        ev, lens = self._replay(n_replays, replay_length, current_state, current_action, True)
        sa = ev['sa'].astype(np.int64)
        live = np.arange(replay_length)[None, None, :] < lens[:, :, None]
        fill = lambda a, v: np.where(live, a, v)      # noqa: E731
        return {'state': fill(sa & 0xFFFF, -1), 'action': fill((sa >> 16) & 0xFF, -1),
                'reward': fill(ev['reward'], np.float32(np.nan)),
                'next_state': fill(ev['next'].astype(np.int64), -1),
                'terminal': fill((sa >> 24) & 1, -1), 'length': lens.astype(np.int64)}

    def retrieve_random_batch(self, number_of_experiences: int, mask) -> list:
        """memory/sfma.py:375-416: uniform draws over the unmasked experiences (one vector draw of
        the memory stream)."""
        m, dev = self._mem()
        n4 = self.nb_states * self.nb_actions
        probs = np.ones(n4) * np.asarray(mask).astype(int)
        assert probs.shape == (n4,), 'mask: one entry per experience, index a * S + s'
        probs /= np.sum(probs)
        if np.isnan(probs).any():
            raise ValueError('probabilities contain NaN')
        cdf = np.cumsum(probs)
        cdf /= cdf[-1]
        cdf_d = torch.as_tensor(cdf, device=dev)
        k = int(number_of_experiences)
        events = torch.zeros((m.n, max(k, 1) * _lib.SFMA_EVENT_BYTES), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().cobel_sfma_random_batch(C.byref(m), k, _lib.ptr(cdf_d),
                                                      _lib.ptr(events), _lib.current_stream(dev)))
        ev = events.cpu().numpy().view(EVENT).reshape(m.n, max(k, 1))[:, :k]
        out = [self._experiences(ev[i]) for i in range(m.n)]
        return out[0] if len(out) == 1 else out
