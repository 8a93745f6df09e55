"""Helpers shared by the tests of SFMAMemory's own methods (store / replay / retrieve_random_batch):
the restatement completed by the two pieces oracle/sfma_loop.py leaves out, the scripts of memory
calls the fixture records, and one driver that runs such a script on any memory (the reference's,
the restatement, the device one) and records it the same way."""
import json

import numpy as np

from oracle.sfma_loop import RefSFMAMemory

SWITCHES = ('mode', 'deterministic', 'recency', 'C_normalize', 'D_normalize', 'R_normalize',
            'reward_mod_local', 'reward_mod', 'state_mod', 'error_mod_local', 'error_mod',
            'decay_strength', 'decay_inhibition', 'reward_modulation', 'beta', 'blend',
            'interpolation_fwd', 'interpolation_rev', 'R_threshold', 'C_step', 'I_step')


class _ActionGiven:
    """A generator whose ``integers`` hands out the given action without drawing: the reference
    skips the draw when ``current_action`` is passed (memory/sfma.py:261-264)."""

    def __init__(self, rng, action):
        self._rng, self._action = rng, action

    def integers(self, *a, **k):
        return self._action

    def __getattr__(self, name):
        return getattr(self._rng, name)


class RefMemory(RefSFMAMemory):
    """RefSFMAMemory plus error modulation in ``store`` (memory/sfma.py:225-233) and
    ``current_action`` in ``replay`` (:261-264)."""
    error_mod_local = error_mod = False

    def store(self, s, a, r, ns, nt, td=None):
        state_mod, self.state_mod = self.state_mod, False     # (it comes after the error modulation)
        try:
            super().store(s, a, r, ns, nt)
        finally:
            self.state_mod = state_mod
        if self.error_mod_local:
            self.C[self.S * a + s] += np.abs(td)
        if self.error_mod:
            self.C += np.abs(td) * np.tile(self.D[ns], self.A)
        if self.state_mod:
            self.C[[s + self.S * k for k in range(self.A)]] += 1.0

    def replay(self, length, current_state=None, current_action=None):
        if current_action is None:
            return super().replay(length, current_state)
        rng = self.rng
        self.rng = _ActionGiven(rng, current_action)
        try:
            return super().replay(length, current_state)
        finally:
            self.rng = rng


def walk_stores(next_table, reward, terminal, starts, n, seed, repeat=None):
    """``n`` stores along a seeded random walk of a world: rows [s, a, r, ns, nonterminal, td].
    ``repeat`` = (position, times): the experience at that position is stored again that often."""
    rng = np.random.default_rng(seed)
    rows, s = [], int(starts[0])
    while len(rows) < n:
        a = int(rng.integers(4))
        ns = int(next_table[s, a])
        end = int(terminal[ns])
        rows.append([s, a, float(reward[ns]), ns, 1 - end, float(np.round(rng.normal(), 3))])
        s = int(starts[int(rng.integers(len(starts)))]) if end else ns
    if repeat:
        at, times = repeat
        rows[at + 1:at + 1] = [list(rows[at]) for _ in range(times)]
    return rows[:n]


def script_for(stores, start, modes, late, length=10):
    """The calls of one fixture case: half of the stores, a replay with the state given and one
    with the state None under every mode (up to here the plain restatement of oracle/sfma_loop.py
    covers every call), one with the action given under every mode, the switches ``late`` (error
    modulation), the other half of the stores, then deterministic and recency replays and one
    masked random batch."""
    half = len(stores) // 2
    ops = [['store'] + row for row in stores[:half]]
    for mode in modes:
        ops += [['set', 'mode', mode], ['replay', length, start, None], ['replay', length, None, None]]
    for k, mode in enumerate(modes):
        ops += [['set', 'mode', mode], ['replay', length - 3, start, k % 4]]
    ops += [['set', k, v] for k, v in late.items()]
    ops += [['store'] + row for row in stores[half:]]
    ops += [['set', 'mode', 'default'], ['set', 'deterministic', True], ['replay', length, start, None],
            ['replay', length, None, 1], ['set', 'deterministic', False], ['set', 'recency', True],
            ['replay', length, start, None], ['replay', length, None, None],
            ['set', 'mode', 'reverse'], ['replay', length, None, 3], ['set', 'recency', False],
            ['random', 7]]
    return ops


def random_mask(n4):
    mask = np.ones(n4, dtype=bool)
    mask[::3] = False
    mask[5::7] = False
    return mask


class Memory:
    """The calls of a script on one kind of memory.  Subclasses give ``store``, ``replay``,
    ``random``, ``set`` and ``snapshot`` -> (C, T, I, index of the memory stream)."""


class OracleMemory(Memory):
    def __init__(self, mem):
        self.mem = mem

    def set(self, name, value):
        assert name in SWITCHES
        setattr(self.mem, name, value)

    def store(self, s, a, r, ns, nt, td):
        self.mem.store(s, a, r, ns, nt, td)

    def replay(self, length, state, action):
        return [[float(x) for x in e] for e in self.mem.replay(length, state, action)]

    def random(self, n, mask):
        return [[float(x) for x in e] for e in self.mem.retrieve_random_batch(n, mask)]

    def snapshot(self):
        m = self.mem
        return m.C.copy(), m.T.copy(), m.I.copy(), m.rng.index

    def tables(self):
        m = self.mem
        return (np.array(m.rewards, dtype=np.float64), np.array(m.states, dtype=np.int64),
                np.array(m.terminals, dtype=np.int64))


class DictMemory(OracleMemory):
    """A memory with the reference's own signatures (experience dicts): the reference's class, or
    the device class (``pick``: the instance looked at, of ``n`` that all get the same calls)."""

    def __init__(self, mem, pick=None, index=None):
        self.mem, self.pick, self._index = mem, pick, index

    def _mine(self, x):
        return x if self.pick is None else x[self.pick]

    def store(self, s, a, r, ns, nt, td):
        self.mem.store({'state': s, 'action': a, 'reward': r, 'next_state': ns, 'terminal': nt,
                        'td': td})

    @staticmethod
    def _rows(exps):
        return [[float(e[k]) for k in ('state', 'action', 'reward', 'next_state', 'terminal')]
                for e in exps]

    def replay(self, length, state, action):
        return self._rows(self._mine(self.mem.replay(length, state, action)))

    def random(self, n, mask):
        return self._rows(self._mine(self.mem.retrieve_random_batch(n, mask)))

    def snapshot(self):
        m = self.mem
        return (np.array(self._mine(m.C), dtype=np.float64), np.array(self._mine(m.T), dtype=np.float64),
                np.array(self._mine(m.I), dtype=np.float64), self._index(m))

    def tables(self):
        m = self.mem
        return (np.array(self._mine(m.rewards), dtype=np.float64),
                np.array(self._mine(m.states), dtype=np.int64),
                np.array(self._mine(m.terminals), dtype=np.int64))


def run_script(mem: Memory, ops) -> dict:
    """Run the calls and record them: per call C, T, I and the stream index after it; every
    returned experience as a row [call, s, a, r, ns, flag]; the model tables at the end."""
    C, T, I, idx, rows = [], [], [], [], []         # noqa: E741
    n4 = None
    for k, op in enumerate(ops):
        kind = op[0]
        if kind == 'set':
            mem.set(op[1], op[2])
        elif kind == 'store':
            s, a, r, ns, nt, td = op[1:]
            mem.store(int(s), int(a), float(r), int(ns), int(nt), float(td))
        elif kind == 'replay':
            rows += [[k] + e for e in mem.replay(op[1], op[2], op[3])]
        elif kind == 'random':
            rows += [[k] + e for e in mem.random(op[1], random_mask(n4))]
        c, t, i, x = mem.snapshot()
        n4 = len(c)
        C.append(c), T.append(t), I.append(i), idx.append(x)
    rw, st, tm = mem.tables()
    return {'C': np.array(C), 'T': np.array(T), 'I': np.array(I),
            'index': np.array(idx, dtype=np.int64),
            'replayed': np.array(rows, dtype=np.float64).reshape(-1, 6),
            'rewards': rw, 'states': st.astype(np.int16), 'terminals': tm.astype(np.int8)}


RECORD_KEYS = ('C', 'T', 'I', 'index', 'replayed', 'rewards', 'states', 'terminals')


def dumps(ops) -> np.ndarray:
    return np.array(json.dumps(ops))


def loads(a) -> list:
    return json.loads(str(a))


def assert_same_record(got: dict, want, keys=RECORD_KEYS, what=''):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError('%s %s differs first at %s: %r != %r'
                                 % (what, k, bad.tolist(), g[tuple(bad)], w[tuple(bad)]))
