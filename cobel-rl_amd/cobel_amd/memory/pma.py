"""Memory module of the PMA agent — ``cobel.memory.PMAMemory`` (memory/pma.py:20-496).

Same constructor, attributes, switches and methods as the reference.  ``replay``, ``store`` and
``update_sr`` are device calls (``cobel_pma_replay`` / ``cobel_pma_store`` / ``cobel_pma_update_sr``,
csrc/pma.hip); inside ``PMA.train`` the stores and the start-of-trial replay are part of the trial
kernel (``cobel_pma_trial``).  A memory is bound to a device by the agent's first session or,
without an agent, by ``bind``.  Every table is float64, as the reference's are.  The host
plumbing shared with ``SFMAMemory`` (``bind``, argument checks, records) is memory/_device.py's.

The observables of the model are device calls of their own (csrc/pma_gain.hip), the expressions the
replay kernel evaluates every round, bit for bit, on tables read in place — so one form serves
the default and the wide memory, up to 1 024 states:

  ``compute_gain_batch(q_function, action_mask)``   the gain of every one-step backup, [A * S]
  ``compute_gain(q_function, action_mask, updates)``   the gain of given n-step updates, of up to
                                                    ``_lib.PMA_MAX_SEQ`` steps each
  ``action_probs_batch(q_function, action_mask=None)``   normalised epsilon-greedy rows of any table
  ``update_q(q_function, update)``                  the n-step update, in place

``q_function`` is one [S, A] table for every instance or [N, S, A]; results are NumPy for a memory
of one instance and device tensors with a leading instance axis for several.  None of them draws a
number or moves a counter.  ``equal_gain`` does not touch them: the reference applies it in
``replay``.

Tables (one leading instance axis on the device; the attributes return NumPy snapshots, squeezed
for one instance, and assigning uploads):

  ``rewards``      float64 [S, A]        ``states`` / ``terminals``  int [S, A]
  ``T`` / ``SR``   float64 [S, S]        ``update_mask``             bool [A * S], index a * S + s

The initial ``T`` and ``SR`` are the reference's NumPy expressions evaluated on the host, so until
the first ``update_sr()`` the SR is the reference's bit for bit.

``compute_need(None)`` — |v| for the unit-2-norm left eigenvector v of T for the eigenvalue nearest
1 — has two modes, chosen by the attribute ``offline_need``:

  ``'host'``    (default) the reference's expression: T is downloaded, ``scipy.linalg.eig`` runs once
                per instance and the vectors are uploaded as need rows.
  ``'device'``  ``cobel_pma_stationary`` (csrc/pma_need.hip): T is row-stochastic, so v is its
                stationary distribution divided by its 2-norm, and one float64 Gaussian elimination
                with partial pivoting of ``(I - T + 1 1^T / S)^T x = 1 / S`` per instance gives it:
                no transfer, no host work, the same bits from the same T.  ``replay`` hands the
                states to the kernel as its selection and the need tensor straight on to
                ``cobel_pma_replay``.  ``need_status`` [N] int32 is the status of the last call.

The two agree to the accuracy either has (both are backward-stable solves; docs/MEASUREMENTS.md
gives the errors against an 80-bit solution), not bit for bit, so a replay may break a near-tie of
``gain * need`` differently.  Where the eigenvalue 1 of T is multiple (several closed classes) the
reference returns whichever vector of the eigenspace LAPACK's iteration ends on; the device mode
returns a defined one: the elimination meets a pivot that is exactly zero (or ends on values that
are not finite), reports status 1 and returns ``1 / sqrt(S)`` in every component.  In the default
form the elimination runs in LDS.  With ``wide=True`` T and SR leave no room for an S x S workspace
there: ``PMAMemory(..., wide=True, need_workspace=k)`` keeps the elimination workspaces of k
instances in device memory (about 8 * S * S bytes each, 8 MiB at 1 024 states; clipped to the
instance count at bind) and ``cobel_pma_stationary_wide`` (csrc/pma_need_wide.hip) does the same
solve on them, the same operations in the same order, k instances at a time.  Without a workspace
(``need_workspace=0``, the default) ``offline_need = 'device'`` raises ``NotImplementedError`` on a
wide memory.

Draws: the memory's generator is stream ``STREAM_PMA_MEMORY`` of (seed, instance) at ``counter``;
the extension actions come from the memory's own policy object — stream ``STREAM_PMA_POLICY`` at
``policy.counter`` unless that object also acts for an agent.

Per-instance parameter sets.  ``learning_rate``, ``learning_rate_q``, ``learning_rate_T``, ``gamma``,
``gamma_q``, ``min_gain`` and the policy's ``epsilon`` take a scalar or one entry per instance (any
other shape is the ``AssertionError`` of ``_device.PER_INSTANCE_SHAPE``): a parameter sweep rides
on the instance axis of one launch (``optimizer.grid_search.spread_over_instances``).  With an
array in any of them ``_fill_params`` turns the distinct rows into ``cobel_pma_param_set_t``
records, gives every instance the index of its row and holds the power tables per set; every
method that reads a parameter honours them (``store``, ``replay``, ``update_sr``,
``compute_gain_batch``, ``compute_gain``, ``update_q``; ``action_probs_batch`` then takes
[N, rows, A]).  The switches (``equal_need``, ``equal_gain``, ``ignore_barriers``, ``allow_loops``,
``min_gain_mode``, ``wide``, ``need_workspace``, ``offline_need``) and the replay length are
launch-wide: an array there is a ``NotImplementedError`` naming the attribute.  As in the
reference the constructor's ``gamma`` gives the initial ``SR`` — an array one host inverse per
distinct value, [N, S, S] — and a later assignment to ``gamma`` only reaches ``update_sr()``.

Two forms.  The default serves worlds of up to 128 states.  ``PMAMemory(..., wide=True)`` selects the
wide form of the kernels: up to 1 024 states and whatever fits 160 KiB of LDS (32 x 32 with four
actions does, with eight it does not), ``update_sr`` by the blocked kernels on the SR in device
memory.  It is opt-in because of its memory: ``T`` and ``SR`` take 8 * S * S bytes each per
instance — 16 MiB per instance at 1 024 states, 16 GiB for a vectorised run of 1 024 instances.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import _device
from .sfma import refuse_arrays

RECORD = np.dtype([('state', '<i4'), ('action', '<i4'), ('next_state', '<i4'),
                   ('terminal', '<i4'), ('reward', '<f8')])

_TABLES = {'rewards': (torch.float64, np.float64), 'states': (torch.int32, np.int64),
           'terminals': (torch.int32, np.int64), 'T': (torch.float64, np.float64),
           'SR': (torch.float64, np.float64), 'update_mask': (torch.uint8, bool)}


# the attributes that take a scalar or one entry per instance, in the order of the memory's seven
# doubles of a cobel_pma_param_set_t (_lib.PMA_SET_MEMORY); the seventh is the policy's epsilon
SET_ATTRIBUTES = ('learning_rate', 'learning_rate_q', 'learning_rate_T', 'gamma', 'gamma_q',
                  'min_gain')
# launch-wide: they change the code path (the switches) or the shape of the launch
LAUNCH_WIDE = ('equal_need', 'equal_gain', 'ignore_barriers', 'allow_loops', 'min_gain_mode', 'wide',
               'need_workspace', 'offline_need')
# the agent part of a set where the memory is called on its own: PMA's defaults, no exploration
AGENT_DEFAULTS = (0.9, 0.99, 0.0)
POW_ROWS = 34      # the least length of a power table: a replay of the default batch and one more


def launch_wide(value, owner: str, name: str):
    """A length (batch, replay length) serves the whole launch: an array is refused by name."""
    if np.ndim(value) > 0:
        raise NotImplementedError('%s.%s is launch-wide: one value for all instances, not an array'
                                  % (owner, name))
    return int(value)


def _table(name: str):
    tdt, ndt = _TABLES[name]

    def get(self):
        if self._dev is None:
            return self._host[name]
        a = self._dev[name].cpu().numpy().astype(ndt)
        return a[0] if a.shape[0] == 1 else a

    def put(self, value) -> None:
        shape = self._shapes[name]
        if self._dev is None:
            v = np.array(value, dtype=ndt)
            self._host[name] = v.reshape(shape if v.size == int(np.prod(shape)) else (-1,) + shape)
            return
        t = self._dev[name]
        v = np.asarray(value.cpu().numpy() if torch.is_tensor(value) else value)
        v = v.astype(ndt).reshape((-1,) + shape)
        t.copy_(torch.as_tensor(np.ascontiguousarray(v), device=t.device).to(tdt).expand_as(t))

    return property(get, put)


class PMAMemory(_device.DeviceMemory):
    def __init__(self, sas, policy, learning_rate: float = 0.9, learning_rate_q: float = 0.9,
                 gamma: float = 0.9, gamma_q: float = 0.9, rng=None, wide: bool = False,
                 need_workspace: int = 0) -> None:
        self.rng = rng
        self.wide = bool(launch_wide(wide, 'PMAMemory', 'wide'))
        self.need_workspace = launch_wide(need_workspace, 'PMAMemory', 'need_workspace')
        if self.need_workspace < 0 or (self.need_workspace and not self.wide):
            raise ValueError(
                'PMAMemory: need_workspace = %d — the number of instances whose elimination '
                'workspaces the wide form (wide=True) holds in device memory; the default form '
                'solves in LDS and takes none' % self.need_workspace)
        self.sas = np.asarray(sas)
        self.policy = policy
        self.learning_rate = learning_rate
        self.learning_rate_q = learning_rate_q
        self.learning_rate_T = 0.9
        self.gamma = gamma
        self.gamma_q = gamma_q
        self.nb_states = S = int(self.sas.shape[0])
        self.nb_actions = A = int(self.sas.shape[1])
        if self.wide:
            self._check_wide(S, A)
        elif S > _lib.PMA_MAX_STATES or A > _lib.PMA_MAX_ACTIONS:
            raise NotImplementedError(
                'PMAMemory: %d states and %d actions — this version serves worlds of up to %d '
                'states and %d actions' % (S, A, _lib.PMA_MAX_STATES, _lib.PMA_MAX_ACTIONS))
        self.min_gain = 10 ** -6
        self.min_gain_mode = 'original'
        self.equal_need = False
        self.equal_gain = False
        self.ignore_barriers = True
        self.allow_loops = False
        self._offline_need = 'host'
        self.need_status = None
        # memory/pma.py:135-146, on the host
        states = np.zeros((S, A)).astype(int)
        T = np.sum(self.sas, axis=1) / A
        self._host = {
            'rewards': np.zeros((S, A)), 'states': states,
            'terminals': np.zeros((S, A)).astype(int), 'T': np.array(T, dtype=np.float64),
            'SR': self._initial_sr(T, self.gamma),
            'update_mask': states.flatten(order='F') != np.tile(np.arange(S), A),
        }
        self._shapes = {'rewards': (S, A), 'states': (S, A), 'terminals': (S, A), 'T': (S, S),
                        'SR': (S, S), 'update_mask': (A * S,)}
        self._psets, self._held, self._tail = {}, None, None
        self._dev = None
        self._need_work = None
        self.counter = None
        self.seed, self.instance_base = 0, 0
        self._pows = None

    @staticmethod
    def _initial_sr(T, gamma):
        """memory/pma.py:141 — ``inv(I - gamma T)`` by NumPy on the host from the constructor's
        gamma: [S, S], or for an array of gammas one inverse per distinct value, [N, S, S] (one
        entry: [S, S], as every table of one instance)."""
        eye = np.eye(T.shape[0])
        if np.ndim(gamma) == 0:
            return np.linalg.inv(eye - gamma * T)
        g = np.asarray(gamma, dtype=np.float64)
        assert g.ndim == 1, _device.PER_INSTANCE_SHAPE
        inverse = {v: np.linalg.inv(eye - v * T) for v in sorted(set(g.tolist()))}
        sr = np.array([inverse[v] for v in g.tolist()])
        return sr[0] if len(sr) == 1 else sr

    @staticmethod
    def _check_wide(S: int, A: int) -> None:
        """The wide plan's word on a world (replay length 0: the tables alone)."""
        out = (C.c_int32 * 4)()
        if _lib.lib().cobel_pma_plan_wide(S, A, 0, C.byref(out)) != _lib.OK:
            raise NotImplementedError(
                'PMAMemory(wide=True): %d states and %d actions — the default form serves up to %d '
                'states and %d actions, the wide form up to %d states within 160 KiB of LDS (%s)'
                % (S, A, _lib.PMA_MAX_STATES, _lib.PMA_MAX_ACTIONS, _lib.PMA_WIDE_MAX_STATES,
                   _lib.lib().cobel_last_error().decode('utf-8', 'replace')))

    def _need_work_bytes(self) -> int:
        """Bytes of one instance's elimination workspace (``cobel_pma_plan_need_wide``)."""
        out = (C.c_int64 * 4)()
        _lib.check(_lib.lib().cobel_pma_plan_need_wide(self.nb_states, C.byref(out)))
        return int(out[0])

    @property
    def offline_need(self) -> str:
        """Where ``compute_need(None)`` runs: ``'host'`` (``scipy.linalg.eig``, the default) or
        ``'device'`` (``cobel_pma_stationary``; on a wide memory with a ``need_workspace``,
        ``cobel_pma_stationary_wide``)."""
        return self._offline_need

    @offline_need.setter
    def offline_need(self, value) -> None:
        launch_wide(0 if np.ndim(value) == 0 else value, 'PMAMemory', 'offline_need')
        if value not in ('host', 'device'):
            raise ValueError("offline_need is 'host' or 'device', not %r" % (value,))
        if value == 'device' and self.wide and not self.need_workspace:
            raise NotImplementedError(
                "PMAMemory(wide=True): offline_need = 'device' serves the default form, worlds of "
                "up to %d states; the wide form keeps compute_need(None) on the host unless it "
                "was built with a need_workspace" % _lib.PMA_MAX_STATES)
        self._offline_need = value

    rewards, states, terminals = _table('rewards'), _table('states'), _table('terminals')
    T, SR, update_mask = _table('T'), _table('SR'), _table('update_mask')

    # -- device state ---------------------------------------------------------------------------
    def _bind(self, n_envs: int, device) -> None:
        if self._dev is not None:
            assert self.n_envs == n_envs, 'a memory stays bound to the instance count it first saw'
            return
        refuse_arrays(self, LAUNCH_WIDE)
        held = min(self.need_workspace, n_envs)
        work = held * self._need_work_bytes() if held else 0
        if self.wide and torch.device(device).type == 'cuda':
            need = n_envs * self.nb_states ** 2 * 16 + work
            free = torch.cuda.mem_get_info(device)[0]
            if need > free:
                raise MemoryError(
                    'PMAMemory(wide=True): T and SR of %d instances of %d states and the need '
                    'workspaces of %d take %d bytes (%.1f GiB), %d bytes of device memory are free'
                    % (n_envs, self.nb_states, held, need, need / 2.0 ** 30, free))
        dev = {}
        for name, (tdt, _) in _TABLES.items():
            h = np.ascontiguousarray(self._host[name])
            t = torch.as_tensor(h, device=device).to(tdt)
            if h.ndim == len(self._shapes[name]):
                t = t.unsqueeze(0)
            else:       # (a table with an instance axis already: the SR of an array of gammas)
                assert h.shape[0] == n_envs, _device.PER_INSTANCE_SHAPE
            dev[name] = t.expand((n_envs,) + self._shapes[name]).contiguous()
        self._dev = dev
        self._need_work = torch.empty(work, dtype=torch.uint8, device=device) if work else None
        self.n_envs = n_envs
        self.counter = torch.zeros(n_envs, dtype=torch.int32, device=device)

    @property
    def device(self):
        return None if self._dev is None else self._dev['T'].device

    def _policy_counter(self):
        pol, dev = self.policy, self.device
        if pol.stream is None:
            pol.stream = _lib.STREAM_PMA_POLICY
        if pol.counter is None or pol.counter.numel() != self.n_envs or pol.counter.device != dev:
            pol.counter = torch.zeros(self.n_envs, dtype=torch.int32, device=dev)
        return pol.counter

    def _power_tables(self, length: int):
        """gamma ** k and gamma_q ** k, k = 0 .. length, by Python's ``**`` (memory/pma.py:310,
        :315, :485, :491): constants, not arithmetic on the data path."""
        key = (float(self.gamma), float(self.gamma_q))
        if self._pows is None or self._pows[0] != key or self._pows[1].shape[1] <= length:
            n = max(length + 1, POW_ROWS)
            tab = np.array([[self.gamma ** k for k in range(n)],
                            [self.gamma_q ** k for k in range(n)]], dtype=np.float64)
            self._pows = (key, torch.as_tensor(tab, device=self.device))
        return self._pows[1]

    def _fill_params(self, x, length: int = 0, agent=None):
        """The seven doubles and the two power tables of the ``cobel_pma_mem_t`` at the head of
        ``x`` (a ``cobel_pma_mem_sets_t``) and the sets in its tail — and, for the
        agent's launcher and ``PMA.update_q``, ``agent = (learning rate, gamma, epsilon)`` — as
        scalars, or, if any of them has one entry per instance, as parameter sets: the distinct
        rows become ``cobel_pma_param_set_t`` records (cached by the bytes of the columns), every
        instance gets the index of its row, the power tables hold one row per set (regrown when
        ``length`` exceeds them) and the scalar fields hold set 0's values as placeholders.
        Returns None for a scalar launch, else what is held: ``first`` (set 0's ten values) and
        the tables ``gamma_pow``, ``gamma_q_pow`` and ``agent_pow`` (the agent's ``gamma ** k``),
        [sets, pow_len] each."""
        refuse_arrays(self, LAUNCH_WIDE)
        m = x.mem
        vals = tuple(getattr(self, a) for a in SET_ATTRIBUTES) + (self.policy.epsilon,)
        cols = _device.param_columns(vals + (tuple(agent) if agent is not None else ()), self.n_envs)
        if cols is None:
            for name, v in zip(_lib.PMA_SET_MEMORY, vals):
                setattr(m, name, float(v))
            pows = self._power_tables(length)
            m.gamma_pow, m.gamma_q_pow = pows[0].data_ptr(), pows[1].data_ptr()
            m.pow_len = pows.shape[1]
            return None
        if agent is None:          # the memory's own calls: the agent part at its defaults
            cols = np.concatenate([cols, np.broadcast_to(AGENT_DEFAULTS, (self.n_envs, 3))], axis=1)
        who = 'agent' if agent is not None else 'memory'
        held = self._psets.setdefault(who, dict(key=None, sets=None, index=None, n=0, first=None,
                                                rows=None, gamma_pow=None, gamma_q_pow=None,
                                                agent_pow=None))

        def fill(rows):
            sets = (_lib.PMAParamSet * len(rows))()
            for k, row in enumerate(rows):
                _lib.check(_lib.lib().cobel_pma_param_set_fill(
                    C.byref((C.c_double * 7)(*row[:7])), float(row[7]), float(row[8]),
                    float(row[9]), C.byref(sets[k])))
            held['rows'], held['gamma_pow'] = np.array(rows), None
            return sets
        new = _device.param_sets(np.ascontiguousarray(cols), held['key'], fill, self.device)
        if new is not None:
            held['key'], held['sets'], held['index'], held['n'], held['first'] = new
        if held['gamma_pow'] is None or held['gamma_pow'].shape[1] <= length:
            n = max(length + 1, POW_ROWS)     # (Python's **, as _power_tables: constants)
            for name, c in (('gamma_pow', 3), ('gamma_q_pow', 4), ('agent_pow', 8)):
                tab = np.array([[float(row[c]) ** k for k in range(n)] for row in held['rows']],
                               dtype=np.float64)
                held[name] = torch.as_tensor(tab, device=self.device)
        for name, v in zip(_lib.PMA_SET_MEMORY, held['first']):     # placeholders: set 0's values
            setattr(m, name, float(v))
        m.gamma_pow, m.gamma_q_pow = _lib.ptr(held['gamma_pow']), _lib.ptr(held['gamma_q_pow'])
        m.pow_len = held['gamma_pow'].shape[1]
        x.param_sets, x.param_index = _lib.ptr(held['sets']), _lib.ptr(held['index'])
        x.n_param_sets = held['n']
        return held

    def flags(self) -> int:
        return ((_lib.PMA_EQUAL_NEED if self.equal_need else 0) |
                (_lib.PMA_EQUAL_GAIN if self.equal_gain else 0) |
                (_lib.PMA_IGNORE_BARRIERS if self.ignore_barriers else 0) |
                (_lib.PMA_ALLOW_LOOPS if self.allow_loops else 0) |
                (_lib.PMA_GAIN_ORIGINAL if self.min_gain_mode == 'original' else 0) |
                (_lib.PMA_WIDE if self.wide else 0))

    def _mem(self, q=None, mask_bits=None, length: int = 0, agent=None):
        """The ``cobel_pma_mem_t`` of a call (``_fill_params`` says what ``agent`` is).  It is the
        head of a ``cobel_pma_mem_sets_t``, which stays in ``self._tail``; with parameter sets its
        flags carry ``PMA_SETS`` and the entry points read the sets behind it.  What
        ``_fill_params`` returned stays in ``self._held`` for the caller."""
        assert self._is_bound, _device.NOT_BOUND
        d = self._dev
        self._tail = x = _lib.PMAMemSets()
        m = x.mem               # (a view: it shares x's memory and keeps x alive)
        m.q = _lib.ptr(q)
        m.rewards, m.states, m.terminals = (_lib.ptr(d['rewards']), _lib.ptr(d['states']),
                                            _lib.ptr(d['terminals']))
        m.T, m.SR, m.update_mask = _lib.ptr(d['T']), _lib.ptr(d['SR']), _lib.ptr(d['update_mask'])
        m.action_mask = _lib.ptr(mask_bits)
        m.mem_ctr, m.pol_ctr = _lib.ptr(self.counter), _lib.ptr(self._policy_counter())
        self._held = self._fill_params(x, length, agent)
        m.n, m.n_states, m.n_actions = self.n_envs, self.nb_states, self.nb_actions
        m.instance_base, m.pol_stream = self.instance_base, self.policy.stream
        m.flags = self.flags() | (_lib.PMA_SETS if self._held is not None else 0)
        m.seed = self.seed
        return m

    def launch_plan(self, replay_length: int = 32) -> list:
        """(LDS bytes, threads) of a replay / trial workgroup and of an update_sr workgroup."""
        plan = _lib.lib().cobel_pma_plan_wide if self.wide else _lib.lib().cobel_pma_plan
        return list(_device.plan4(plan, self.nb_states, self.nb_actions, int(replay_length)))

    def _per_instance(self, value, name: str, limit: int):
        """scalar / [N] -> int32 [N], range-checked; entries None or < 0 become -1."""
        return _device.per_instance(value, self.n_envs, name, limit, none_as=-1)

    def _mask_bits(self, action_mask):
        if action_mask is None:
            return None
        return torch.as_tensor(_device.mask_bits(action_mask, self.nb_states, self.nb_actions),
                               device=self.device)

    # -- the reference's methods ------------------------------------------------------------------
    def store(self, experience: dict) -> None:
        """memory/pma.py:148-166.  One experience per instance: the values of ``experience`` are
        scalars (the same for all instances) or [N] arrays."""
        m = self._mem()
        S = self.nb_states
        rec = _device.records(experience, self.n_envs, RECORD,
                              {'state': S, 'action': self.nb_actions, 'next_state': S}, none_as=-1)
        exps = torch.as_tensor(rec.view(np.uint8), device=self.device)
        _lib.check(_lib.lib().cobel_pma_store(C.byref(m), _lib.ptr(exps),
                                              _lib.current_stream(self.device)))

    def _replay_device(self, q, mask_bits, length: int, states, need_rows, force_first):
        """One replay per instance IN PLACE on the device tensor ``q`` [N, S, A]: ``states`` int32
        [N] host array or device tensor (-1: the instance's row of ``need_rows`` [N, S], a host
        array or a float64 device tensor) or None (all from ``need_rows``).  Returns the records
        as a uint8 device tensor [N, length * 24]."""
        dev = self.device
        m = self._mem(q, mask_bits, length)
        st_d = None if states is None else torch.as_tensor(states, device=dev)
        if need_rows is None or torch.is_tensor(need_rows):
            nd_d = need_rows
        else:
            nd_d = torch.as_tensor(np.ascontiguousarray(need_rows, dtype=np.float64), device=dev)
        ff_d = None if force_first is None else torch.as_tensor(force_first, device=dev)
        records = torch.zeros((self.n_envs, max(length, 1) * RECORD.itemsize), dtype=torch.uint8,
                              device=dev)
        _lib.check(_lib.lib().cobel_pma_replay(
            C.byref(m), int(length), _lib.ptr(st_d), _lib.ptr(nd_d), _lib.ptr(ff_d),
            _lib.ptr(records), _lib.current_stream(dev)))
        return records

    @staticmethod
    def experiences(records, length: int) -> list:
        """Record tensor -> per instance the reference's list of experience dicts."""
        raw = records.cpu().numpy().view(RECORD)[:, :length]
        return [[{'state': int(e['state']), 'action': int(e['action']), 'reward': float(e['reward']),
                  'next_state': int(e['next_state']), 'terminal': int(e['terminal'])}
                 for e in row] for row in raw]

    def _need_rows(self, states, instances=None):
        """The need vectors [N, S] of the instances whose state is -1 / None (host path), or None
        when every instance names a state."""
        if states is not None and (states >= 0).all():
            return None
        S, n = self.nb_states, self.n_envs
        idx = np.arange(n) if states is None else np.flatnonzero(states < 0)
        need = np.asarray(self.compute_need(None, instances=idx), dtype=np.float64)
        rows = np.zeros((n, S))
        rows[idx] = need.reshape(-1, self.nb_actions * S)[:, :S]
        return rows

    def _need_device(self, select):
        """``cobel_pma_stationary`` (a wide memory: ``cobel_pma_stationary_wide`` on its
        workspace): the need tensor [N, S] (float64, device) with the rows of the instances whose
        entry of ``select`` (int32 [N] device tensor, or None: all) is negative filled in, the
        others zero; ``need_status`` takes the call's status [N]."""
        assert self._is_bound, _device.NOT_BOUND
        dev = self.device
        need = torch.zeros((self.n_envs, self.nb_states), dtype=torch.float64, device=dev)
        self.need_status = torch.zeros(self.n_envs, dtype=torch.int32, device=dev)
        m = self._mem()
        if self.wide:
            if self._need_work is None:
                raise NotImplementedError(
                    'PMAMemory(wide=True): the stationary distribution on the device takes a '
                    'workspace — build the memory with need_workspace >= 1')
            _lib.check(_lib.lib().cobel_pma_stationary_wide(
                C.byref(m), _lib.ptr(select), _lib.ptr(need), _lib.ptr(self.need_status),
                _lib.ptr(self._need_work), self._need_work.numel(), _lib.current_stream(dev)))
        else:
            _lib.check(_lib.lib().cobel_pma_stationary(
                C.byref(m), _lib.ptr(select), _lib.ptr(need), _lib.ptr(self.need_status),
                _lib.current_stream(dev)))
        return need

    def stationary(self, instances=None):
        """The vectors of ``compute_need(None)`` by the device kernel, whatever ``offline_need``
        says: a float64 device tensor [n, S], one row per entry of ``instances`` (default:
        all).  ``need_status`` tells the degenerate ones."""
        if instances is None:
            return self._need_device(None)
        idx = np.asarray(instances, dtype=np.int64).reshape(-1)
        select = np.zeros(self.n_envs, dtype=np.int32)
        select[idx] = -1
        need = self._need_device(torch.as_tensor(select, device=self.device))
        return need[torch.as_tensor(idx, device=self.device)]

    def replay(self, q_function, action_mask, replay_length: int, current_state,
               force_first=None):
        """memory/pma.py:168-267: one replay per instance on a copy of ``q_function`` ([S, A], or
        [N, S, A]).  Returns ``(updates, Q)``: the performed updates as a list of experience dicts
        and the updated copy as a NumPy array for one instance; one list per instance and the
        device tensor [N, S, A] for several.  ``current_state`` / ``force_first`` are scalars or
        [N] arrays; ``current_state=None`` (or an entry None / < 0) takes ``compute_need(None)``:
        with ``offline_need = 'host'`` through the host, with ``'device'`` by
        ``cobel_pma_stationary`` without leaving the device."""
        assert self._is_bound, _device.NOT_BOUND
        n, S, A = self.n_envs, self.nb_states, self.nb_actions
        length = launch_wide(replay_length, 'PMAMemory', 'replay_length')
        if torch.is_tensor(q_function):
            q = q_function.to(device=self.device, dtype=torch.float64)
        else:
            q = torch.as_tensor(np.asarray(q_function, dtype=np.float64), device=self.device)
        q = q.reshape((-1, S, A)).expand((n, S, A)).clone().contiguous()
        states = (None if current_state is None
                  else self._per_instance(current_state, 'current_state', S))
        ff = None if force_first is None else self._per_instance(force_first, 'force_first', S)
        if self._offline_need == 'device':
            rows = None
            if states is None or (states < 0).any():
                states = None if states is None else torch.as_tensor(states, device=self.device)
                rows = self._need_device(states)
        else:
            rows = self._need_rows(states)
        records = self._replay_device(q, self._mask_bits(action_mask), length, states, rows, ff)
        ups = self.experiences(records, length)
        if n == 1:
            return ups[0], q[0].cpu().numpy()
        return ups, q

    # -- the observables: gain maps, n-step gains, action probabilities, update_q -----------------
    def _q_tables(self, q_function, who: str):
        """``q_function`` [S, A] (one table for every instance) or [N, S, A], NumPy or tensor ->
        (float64 device tensor, the ``q_stride`` of the C calls)."""
        S, A = self.nb_states, self.nb_actions
        if torch.is_tensor(q_function):
            q = q_function.to(device=self.device, dtype=torch.float64)
        else:
            q = torch.as_tensor(np.asarray(q_function, dtype=np.float64), device=self.device)
        if tuple(q.shape) == (S, A):
            return q.contiguous(), 0
        if tuple(q.shape) == (self.n_envs, S, A):
            return q.contiguous(), S * A
        raise ValueError('%s: q_function of shape %s — [%d, %d] or [%d, %d, %d] is expected'
                         % (who, tuple(q.shape), S, A, self.n_envs, S, A))

    def _sequences(self, updates: list, who: str):
        """A list of n-step updates (lists of experience dicts of scalars or [N] arrays) as the
        record tensor [rows, len(updates), max_len] — rows = 1 where every value is a scalar, N
        otherwise — with the lengths int32 [rows, len(updates)] (host) and ``max_len``.  An
        instance whose ``state`` entry is None or negative from some step on has a shorter
        sequence."""
        n, S = self.n_envs, self.nb_states
        for update in updates:
            if len(update) == 0:
                raise IndexError('%s: an update without steps (update[-1] of an empty list)' % who)
        max_len = max([len(u) for u in updates], default=1)
        if max_len > _lib.PMA_MAX_SEQ:
            raise NotImplementedError('%s: an update of %d steps — this version serves sequences '
                                      'of up to %d steps' % (who, max_len, _lib.PMA_MAX_SEQ))
        per = any(np.ndim(v) > 0 for u in updates for step in u for v in step.values())
        rows = n if per else 1
        rec = np.zeros((rows, len(updates), max_len), dtype=RECORD)
        lengths = np.zeros((rows, len(updates)), dtype=np.int32)
        limits = {'state': S, 'action': self.nb_actions, 'next_state': S}
        for k, update in enumerate(updates):
            for j, step in enumerate(update):
                rec[:, k, j] = _device.records(step, rows, RECORD, limits, none_as=-1)
            valid = rec['state'][:, k, :len(update)] >= 0
            lengths[:, k] = valid.sum(axis=1)
            if (lengths[:, k] < 1).any() or \
                    (valid != (np.arange(len(update))[None, :] < lengths[:, k, None])).any():
                raise IndexError('%s: the steps of an instance are the first ones of the update, '
                                 'at least one' % who)
        steps = torch.as_tensor(np.ascontiguousarray(rec).view(np.uint8).reshape(-1),
                                device=self.device)
        return steps, lengths, max_len, per

    def compute_gain_batch(self, q_function, action_mask):
        """memory/pma.py:333-386 on the device (``cobel_pma_gain_batch``): the gain of every
        one-step backup, index ``a * S + s``.  ``q_function`` is [S, A] (every instance scores the
        same table) or [N, S, A], NumPy or a device tensor.  Returns NumPy [A * S] for one
        instance, a float64 device tensor [N, A * S] for several."""
        assert self._is_bound, _device.NOT_BOUND
        q, stride = self._q_tables(q_function, 'compute_gain_batch')
        gain = torch.empty((self.n_envs, self.nb_actions * self.nb_states), dtype=torch.float64,
                           device=self.device)
        bits = self._mask_bits(action_mask)
        m = self._mem(None, bits)
        _lib.check(_lib.lib().cobel_pma_gain_batch(C.byref(m), _lib.ptr(q), stride, _lib.ptr(gain),
                                                   _lib.current_stream(self.device)))
        return gain[0].cpu().numpy() if self.n_envs == 1 else gain

    def compute_gain(self, q_function, action_mask, updates: list):
        """memory/pma.py:269-331 on the device (``cobel_pma_gain_seq``): the gain of each n-step
        update of ``updates``, a list of lists of experience dicts whose values are scalars or [N]
        arrays (per-instance steps; a ``state`` of None or < 0 ends that instance's sequence
        early).  Returns NumPy [len(updates)] for one instance, a float64 device tensor
        [N, len(updates)] for several."""
        assert self._is_bound, _device.NOT_BOUND
        q, stride = self._q_tables(q_function, 'compute_gain')
        steps, lengths, max_len, per = self._sequences(updates, 'compute_gain')
        n_seq = len(updates)
        gain = torch.empty((self.n_envs, n_seq), dtype=torch.float64, device=self.device)
        if n_seq == 0:
            return gain[0].cpu().numpy() if self.n_envs == 1 else gain
        bits = self._mask_bits(action_mask)
        m = self._mem(None, bits, max_len)
        _lib.check(_lib.lib().cobel_pma_gain_seq(
            C.byref(m), _lib.ptr(q), stride, _lib.ptr(steps), _lib.ptr(lengths), n_seq, max_len,
            n_seq * max_len if per else 0, _lib.ptr(gain), _lib.current_stream(self.device)))
        return gain[0].cpu().numpy() if self.n_envs == 1 else gain

    def action_probs_batch(self, q_function, action_mask=None):
        """memory/pma.py:423-450 on the device (``cobel_pma_action_probs``): the policy's
        epsilon-greedy probabilities of every row of a [rows, A] table, each row divided by its
        sum; ``action_mask`` is [rows, A] booleans or None.  NumPy in gives NumPy out, a tensor in
        a tensor out.  Needs no bound memory.  With one epsilon per instance ``q_function`` is
        [N, rows, A] and the call is made once per distinct epsilon on the rows of its instances."""
        if np.ndim(self.policy.epsilon) > 0:
            return self._action_probs_per_instance(q_function, action_mask)
        return self._action_probs(q_function, action_mask, float(self.policy.epsilon))

    def _action_probs_per_instance(self, q_function, action_mask):
        eps = np.asarray(self.policy.epsilon, dtype=np.float64)
        is_tensor = torch.is_tensor(q_function)
        q = q_function if is_tensor else np.asarray(q_function, dtype=np.float64)
        assert eps.ndim == 1 and q.ndim == 3 and q.shape[0] == eps.shape[0], \
            _device.PER_INSTANCE_SHAPE
        out = torch.empty_like(q, dtype=torch.float64) if is_tensor else np.empty(q.shape)
        for e in np.unique(eps):
            sel = np.flatnonzero(eps == e)
            idx = torch.as_tensor(sel, device=q.device) if is_tensor else sel
            part = self._action_probs(q[idx].reshape(-1, q.shape[2]),
                                      None if action_mask is None else
                                      np.tile(np.asarray(action_mask.cpu() if torch.is_tensor(
                                          action_mask) else action_mask), (len(sel), 1)), float(e))
            out[idx] = part.reshape((len(sel),) + tuple(q.shape[1:]))
        return out

    def _action_probs(self, q_function, action_mask, epsilon: float):
        is_tensor = torch.is_tensor(q_function)
        if is_tensor and q_function.is_cuda:
            dev = q_function.device
        else:
            dev = self.device or torch.device('cuda', torch.cuda.current_device())
        if is_tensor:
            q = q_function.to(device=dev, dtype=torch.float64).contiguous()
        else:
            q = torch.as_tensor(np.asarray(q_function, dtype=np.float64), device=dev).contiguous()
        if q.dim() != 2 or not 1 <= q.shape[1] <= _lib.PMA_MAX_ACTIONS:
            raise ValueError('action_probs_batch: q_function of shape %s — [rows, A] with up to %d '
                             'actions is expected' % (tuple(q.shape), _lib.PMA_MAX_ACTIONS))
        rows, A = int(q.shape[0]), int(q.shape[1])
        bits = None
        if action_mask is not None:
            mask = action_mask.cpu().numpy() if torch.is_tensor(action_mask) else action_mask
            bits = torch.as_tensor(_device.mask_bits(mask, rows, A), device=dev)
        probs = torch.empty((rows, A), dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().cobel_pma_action_probs(
            _lib.ptr(q), _lib.ptr(bits), rows, A, epsilon, _lib.ptr(probs),
            _lib.current_stream(dev)))
        return probs if is_tensor else probs.cpu().numpy()

    def _update_q_device(self, q, update: list, agent=None) -> None:
        """The n-step update IN PLACE on the device tensor ``q`` [N, S, A]: the memory's
        (``learning_rate_q``, ``gamma_q ** k``) or, with ``agent = (learning rate, gamma,
        epsilon)``, the agent's (its learning rate, ``gamma ** k``).  ``cobel_pma_update_q`` for
        scalars, ``cobel_pma_update_q_sets`` where a parameter has one entry per instance."""
        steps, lengths, max_len, per = self._sequences([update], 'update_q')
        m = self._mem(length=len(update), agent=agent)
        stride, stream = max_len if per else 0, _lib.current_stream(self.device)
        if self._held is not None:
            which = _lib.PMA_Q_MEMORY if agent is None else _lib.PMA_Q_AGENT
            _lib.check(_lib.lib().cobel_pma_update_q_sets(
                C.byref(m), _lib.ptr(q), _lib.ptr(steps), _lib.ptr(lengths), max_len, stride, which,
                _lib.ptr(self._held['agent_pow']), stream))
            return
        if agent is None:
            rate, table = self.learning_rate_q, self._power_tables(len(update))[1]
        else:
            rate = agent[0]
            table = torch.as_tensor(np.array([agent[1] ** k for k in range(len(update) + 1)],
                                             dtype=np.float64), device=self.device)
        _lib.check(_lib.lib().cobel_pma_update_q(
            C.byref(m), _lib.ptr(q), _lib.ptr(steps), _lib.ptr(lengths), max_len, stride,
            float(rate), table.data_ptr(), int(table.numel()), stream))

    def update_q(self, q_function, update: list):
        """memory/pma.py:452-496 on the device (``cobel_pma_update_q``): the n-step update of
        ``update`` (experience dicts of scalars or [N] arrays) with ``learning_rate_q`` and
        ``gamma_q``.  A float64 device tensor [N, S, A] is updated in place and returned; a NumPy
        array ([S, A] for one instance, [N, S, A]) is updated in place as the reference mutates
        its argument, and returned."""
        assert self._is_bound, _device.NOT_BOUND
        n, S, A = self.n_envs, self.nb_states, self.nb_actions
        shape = tuple(q_function.shape) if hasattr(q_function, 'shape') else np.shape(q_function)
        if shape != (n, S, A) and not (n == 1 and shape == (S, A)):
            raise ValueError('update_q: q_function of shape %s — [%d, %d, %d]%s is expected'
                             % (shape, n, S, A, ' or [%d, %d]' % (S, A) if n == 1 else ''))
        if torch.is_tensor(q_function):
            if (q_function.dtype != torch.float64 or q_function.device != self.device
                    or not q_function.is_contiguous()):
                raise ValueError('update_q: a tensor is updated in place — a contiguous float64 '
                                 'tensor on %s is expected' % (self.device,))
            self._update_q_device(q_function, update)
            return q_function
        q = torch.as_tensor(np.asarray(q_function, dtype=np.float64), device=self.device)
        q = q.reshape((n, S, A)).contiguous()
        self._update_q_device(q, update)
        if isinstance(q_function, np.ndarray):
            q_function[...] = q.cpu().numpy().reshape(shape)
            return q_function
        return q.cpu().numpy().reshape(shape)

    def compute_need(self, current_state=None, instances=None):
        """memory/pma.py:388-411.  ``None``: the unit-2-norm stationary vector of T of
        ``instances`` (default: all), tiled ``nb_actions`` times, as NumPy: by
        ``scipy.linalg.eig`` on the host, or with ``offline_need = 'device'`` by the kernel."""
        S, A = self.nb_states, self.nb_actions
        if current_state is None and self._offline_need == 'device':
            out = np.tile(self.stationary(instances).cpu().numpy(), (1, A))
            return out[0] if (instances is None and len(out) == 1) else out
        if current_state is None:
            from scipy import linalg
            T = np.asarray(self.T, dtype=np.float64).reshape(-1, S, S)
            idx = np.arange(T.shape[0]) if instances is None else np.asarray(instances)
            out = []
            for i in idx:
                eig, vec = linalg.eig(T[i], left=True, right=False)
                best = np.argmin(np.abs(eig - 1))
                out.append(np.tile(np.abs(vec[:, best].T), A))
            out = np.array(out)
            return out[0] if (instances is None and len(out) == 1) else out
        SR = np.asarray(self.SR).reshape(-1, S, S)
        cs = np.broadcast_to(np.asarray(current_state, dtype=np.int64), (SR.shape[0],))
        out = np.array([np.tile(SR[i, cs[i]], A) for i in range(SR.shape[0])])
        return out[0] if len(out) == 1 else out

    def update_sr(self) -> None:
        """memory/pma.py:413-415 on the device: SR = inv(I - gamma T) per instance."""
        m = self._mem()
        _lib.check(_lib.lib().cobel_pma_update_sr(C.byref(m), _lib.current_stream(self.device)))

    def compute_update_mask(self) -> None:
        """memory/pma.py:417-421."""
        S, A = self.nb_states, self.nb_actions
        if self._dev is None:
            self._host['update_mask'] = (self._host['states'].flatten(order='F') !=
                                         np.tile(np.arange(S), A))
            return
        st = self._dev['states']
        flat = st.permute(0, 2, 1).reshape(st.shape[0], A * S)
        own = torch.arange(S, device=st.device, dtype=st.dtype).repeat(A)
        self._dev['update_mask'].copy_((flat != own).to(torch.uint8))
