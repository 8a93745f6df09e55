"""Helpers shared by the PMA tests: a plain NumPy restatement of PMAMemory and of the PMA trial loop
driven by ``TapeRNG`` (the same arithmetic, call for call, as memory/pma.py and agent/pma.py of the
reference), the scripts of memory calls the fixture records, and one driver that runs such a script
on any memory (the reference's, the restatement, the device one) and records it the same way."""
import json

import numpy as np

from oracle.philox import STREAM_ENV, STREAM_POLICY, TapeRNG
from oracle.ref_loop import RefEpsilonGreedy, RefGridworld

STREAM_PMA_MEMORY, STREAM_PMA_POLICY = 5, 6
KEYS = ('state', 'action', 'reward', 'next_state', 'terminal')
SWITCHES = ('equal_need', 'equal_gain', 'ignore_barriers', 'allow_loops', 'min_gain',
            'min_gain_mode')


def memory_rngs(seed, inst):
    """(the memory's generator, its policy's generator) of instance ``inst``."""
    return (TapeRNG(seed, inst, STREAM_PMA_MEMORY, double_sub=1),
            TapeRNG(seed, inst, STREAM_PMA_POLICY))


def gauss_jordan(T, gamma):
    """k_pma_update_sr's operations element by element: pivots ascending, no pivoting, the pivot
    row scaled by 1 / pivot, every other element M - col[r] * row[c] (0 - ... in column k)."""
    S = T.shape[0]
    M = np.eye(S) - gamma * T
    for k in range(S):
        inv = 1.0 / M[k, k]
        col = M[:, k].copy()
        row = M[k, :].copy()
        row[k] = 1.0
        row = row * inv
        M[:, k] = 0.0
        M = M - col[:, None] * row[None, :]
        M[k, :] = row
    return M


class RefPMAMemory:
    """memory/pma.py:20-496."""

    def __init__(self, sas, policy, learning_rate=0.9, learning_rate_q=0.9, gamma=0.9, gamma_q=0.9,
                 rng=None, sr_by_elimination=False):
        self.rng, self.policy = rng, policy
        # update_sr by ``gauss_jordan``, the device kernels' operations, not by LAPACK (the
        # constructor's SR below is numpy.linalg.inv on both sides either way)
        self.sr_by_elimination = sr_by_elimination
        # what the replays held, for the tests that ask what a sweep contains: per replay() call
        # whether an extended (n-step, n > 1) sequence was chosen and whether the largest utility
        # was tied so that the draw decided
        self.seen = {'replays': 0, 'extended': 0, 'tied': 0}
        self.learning_rate, self.learning_rate_q, self.learning_rate_T = learning_rate, learning_rate_q, 0.9
        self.gamma, self.gamma_q = gamma, gamma_q
        self.nb_states, self.nb_actions = S, A = sas.shape[0], sas.shape[1]
        self.min_gain, self.min_gain_mode = 10 ** -6, 'original'
        self.equal_need = self.equal_gain = self.allow_loops = False
        self.ignore_barriers = True
        self.rewards = np.zeros((S, A))
        self.states = np.zeros((S, A)).astype(int)
        self.terminals = np.zeros((S, A)).astype(int)
        self.T = np.sum(sas, axis=1) / A
        self.SR = np.linalg.inv(np.eye(S) - self.gamma * self.T)
        self.compute_update_mask()
        self.need_given = None      # tests: the need vector compute_need(None) returns

    def compute_update_mask(self):
        self.update_mask = self.states.flatten(order='F') != np.tile(np.arange(self.nb_states),
                                                                     self.nb_actions)

    def update_sr(self):
        if self.sr_by_elimination:
            self.SR = gauss_jordan(self.T, self.gamma)
        else:
            self.SR = np.linalg.inv(np.eye(self.nb_states) - self.gamma * self.T)

    def store(self, e):
        s, a = e['state'], e['action']
        self.rewards[s][a] += self.learning_rate * (e['reward'] - self.rewards[s][a])
        self.states[s][a] = e['next_state']
        self.terminals[s][a] = e['terminal']
        self.T[s] += self.learning_rate_T * ((np.arange(self.nb_states) == e['next_state']) - self.T[s])

    def _step(self, i):
        s, a = i % self.nb_states, int(i / self.nb_states)
        return {'state': s, 'action': a, 'reward': self.rewards[s, a],
                'next_state': self.states[s, a], 'terminal': self.terminals[s, a]}

    def compute_need(self, current_state=None):
        if current_state is None:
            if self.need_given is not None:
                return np.array(self.need_given, dtype=np.float64)
            from scipy import linalg
            eig, vec = linalg.eig(self.T, left=True, right=False)
            return np.tile(np.abs(vec[:, np.argmin(np.abs(eig - 1))].T), self.nb_actions)
        return np.tile(self.SR[current_state], self.nb_actions)

    def _probs_batch(self, q, mask):
        p = np.array([self.policy.get_action_probs(v, mask[s] if mask is not None else None)
                      for s, v in enumerate(q)])
        return p / np.sum(p, axis=1).reshape(p.shape[0], 1)

    def compute_gain_batch(self, Q, action_mask):
        S, A = Q.shape
        updates = np.tile(Q, (A, 1))
        targets = Q[self.states.flatten(order='F')]
        tmask = np.zeros(updates.shape)
        for a in range(A):
            tmask[S * a:S * (a + 1), a] = 1.0
        q_new = np.copy(updates)
        q_new += (self.learning_rate_q * tmask
                  * (np.tile(self.rewards, (A, 1))
                     + self.gamma_q * np.amax(targets, axis=1).reshape(targets.shape[0], 1)
                     * self.terminals.flatten(order='F').reshape(targets.shape[0], 1)
                     - q_new))
        mask = np.tile(action_mask, (A, 1)) if action_mask is not None else None
        p_old, p_new = self._probs_batch(updates, mask), self._probs_batch(q_new, mask)
        gain = np.sum(p_new * q_new, axis=1) - np.sum(p_old * q_new, axis=1)
        return np.clip(gain, a_min=self.min_gain, a_max=None)

    def compute_gain(self, Q, action_mask, update):
        gain = 0.0
        fv = np.amax(Q[update[-1]['next_state']]) * update[-1]['terminal']
        for s, step in enumerate(update):
            mask = action_mask[step['state']] if action_mask is not None else None
            before = self.policy.get_action_probs(Q[step['state']], mask)
            r = 0.0
            for k in range(len(update) - s):
                r += update[s + k]['reward'] * (self.gamma ** k)
            target = np.copy(Q[step['state']])
            target[step['action']] = r + fv * (self.gamma_q ** (k + 1))
            q_new = Q[step['state']] + self.learning_rate_q * (target - Q[step['state']])
            after = self.policy.get_action_probs(q_new, mask)
            g = np.sum(q_new * after) - np.sum(q_new * before)
            if self.min_gain_mode == 'original':
                g = max(g, self.min_gain)
            gain += g
        return max(gain, self.min_gain)

    def update_q(self, Q, update, lr=None, gamma=None):
        lr = self.learning_rate_q if lr is None else lr
        gamma = self.gamma_q if gamma is None else gamma
        fv = np.amax(Q[update[-1]['next_state']]) * update[-1]['terminal']
        for s, step in enumerate(update):
            r, ok = 0.0, True
            for k in range(len(update) - s):
                if update[s + k]['terminal'] == 0 and s != len(update) - 1:
                    ok = False
                    break
                r += update[s + k]['reward'] * (gamma ** k)
            if not ok:
                break
            td = r + fv * (gamma ** (k + 1))
            td -= Q[step['state']][step['action']]
            Q[step['state']][step['action']] += lr * td
        return Q

    def replay(self, q_function, action_mask, replay_length, current_state, force_first=None):
        S, A = self.nb_states, self.nb_actions
        done, Q, last_seq = [], np.copy(q_function), 0
        extended = tied = False
        for upd in range(replay_length):
            ext, seq = -1, None
            if done:
                ext = done[-1]['next_state']
                loop = any(ext == st['state'] for st in done[last_seq:])
                if not loop or self.allow_loops:
                    mask = action_mask[ext] if action_mask is not None else None
                    ext += int(self.policy.select_action(Q[ext], mask)) * S
                    seq = done[last_seq:] + [self._step(ext)]
            gain = self.compute_gain_batch(Q, action_mask)
            if ext != -1:
                gain[ext] = self.compute_gain(Q, action_mask, seq if seq else [self._step(ext)])
            if self.equal_gain:
                gain.fill(1)
            need = self.compute_need(current_state)
            if self.equal_need:
                need.fill(1)
            utility = gain * need
            if self.ignore_barriers:
                utility *= self.update_mask
            ties = utility == np.amax(utility)
            best = self.rng.choice(np.arange(S * A), p=ties / np.sum(ties))
            tied |= int(np.sum(ties)) > 1 and not (not done and force_first is not None)
            if not done and force_first is not None:
                best = force_first + self.rng.integers(A) * S
            chosen = seq if (seq and best == ext) else [self._step(best)]
            extended |= len(chosen) > 1
            Q = self.update_q(Q, chosen)
            done += [chosen[-1]]
            if ext != best:
                last_seq = upd
        self.seen['replays'] += 1
        self.seen['extended'] += int(extended)
        self.seen['tied'] += int(tied)
        return done, Q


class RefPMA:
    """agent/pma.py:167-353 on a RefGridworld."""

    def __init__(self, n_states, n_actions, policy, memory, learning_rate=0.9, gamma=0.99):
        self.policy, self.M = policy, memory
        self.learning_rate, self.gamma = learning_rate, gamma
        self.Q = np.zeros((n_states, n_actions))
        self.action_mask = np.ones((n_states, n_actions)).astype(bool)
        self.mask_actions = False
        self.update_sr = None      # tests: called instead of M.update_sr() (injects a recorded SR)

    def train(self, env, trials, steps, batch_size=32, no_replay=False, trace=None):
        mask = lambda: self.action_mask if self.mask_actions else None   # noqa: E731
        for _ in range(trials):
            last = None
            state, _ = env.reset()
            if not no_replay:
                rep, self.Q = self.M.replay(self.Q, mask(), batch_size, state)
                if trace is not None:
                    trace['replay_start'].append(rows_of(rep))
                    trace['q_start'].append(self.Q.copy())
            for step in range(steps):
                a = self.policy.select_action(self.Q[state],
                                              self.action_mask[state] if self.mask_actions else None)
                ns, r, end, _, _ = env.step(a)
                e = {'state': state, 'action': int(a), 'reward': float(r), 'next_state': ns,
                     'terminal': 1 - end}
                self.M.update_q(self.Q, [e], self.learning_rate, self.gamma)
                self.M.store(e)
                state = ns
                if end:
                    last = ns
                    break
            if not no_replay:
                (self.update_sr or self.M.update_sr)()
                rep, self.Q = self.M.replay(self.Q, mask(), batch_size, last)
                if trace is not None:
                    trace['sr'].append(self.M.SR.copy())
                    trace['replay_end'].append(rows_of(rep))
            if trace is not None:
                trace['q_end'].append(self.Q.copy())
                trace['steps'].append(step)
                trace['last'].append(-1 if last is None else last)


def new_trace():
    return {k: [] for k in ('replay_start', 'q_start', 'sr', 'replay_end', 'q_end', 'steps', 'last')}


def rows_of(exps):
    return np.array([[float(e[k]) for k in KEYS] for e in exps], dtype=np.float64).reshape(-1, 5)


def make_ref_agent(tabs, sas, seed, inst, gamma_q=0.99, epsilon=0.1, shared_policy=False,
                   sr_by_elimination=False):
    """The restatement's env, agent and memory of instance ``inst`` on the project's streams.
    ``shared_policy``: the memory's policy object is the agent's (one stream for both)."""
    env = RefGridworld(tabs, TapeRNG(seed, inst, STREAM_ENV))
    rm, rp = memory_rngs(seed, inst)
    pol = RefEpsilonGreedy(epsilon, TapeRNG(seed, inst, STREAM_POLICY))
    mem = RefPMAMemory(sas, pol if shared_policy else RefEpsilonGreedy(epsilon, rp), gamma_q=gamma_q,
                       rng=rm, sr_by_elimination=sr_by_elimination)
    S, A = sas.shape[0], sas.shape[1]
    agent = RefPMA(S, A, pol, mem)
    return env, agent, mem


# -- worlds ---------------------------------------------------------------------------------------
DEMO_WALLS = [(3, 4), (4, 3), (8, 9), (9, 8), (13, 14), (14, 13), (18, 19), (19, 18)]


def demo_world():
    """The world of the reference's demo_pma.py: 5 x 5, four walls, start 12, reward 10 at 4."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    w = make_gridworld(5, 5, terminals=[4], rewards=np.array([[4, 10]]), goals=[4],
                       invalid_transitions=list(DEMO_WALLS))
    w['starting_states'] = np.array([12])
    return w


def small_world():
    """3 x 4 with one wall: S x A = 48, less than one wavefront."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    w = make_gridworld(3, 4, terminals=[3], rewards=np.array([[3, 10]]), goals=[3],
                       invalid_transitions=[(5, 6), (6, 5)])
    w['starting_states'] = np.array([8])
    return w


def seeded_world(height, width, seed):
    """A world the fixture does not hold: seeded walls between neighbours, a rewarded corner."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    rng = np.random.default_rng(seed)
    S = height * width
    walls = []
    for s in rng.choice(S - 1, size=S // 5, replace=False):
        s = int(s)
        if (s + 1) % width and s + 1 != width - 1:
            walls += [(s, s + 1), (s + 1, s)]
    goal = width - 1
    w = make_gridworld(height, width, terminals=[goal], rewards=np.array([[goal, 10]]), goals=[goal],
                       invalid_transitions=walls)
    w['starting_states'] = np.array([S // 2])
    return w


WORLDS = {'demo_5x5': demo_world, 'small_3x4': small_world}


def sas_of(nxt):
    """Dense ``sas[S, A, S]`` of a deterministic successor table ``next[S, A]``, any action count."""
    nxt = np.asarray(nxt).astype(np.int64)
    S, A = nxt.shape
    sas = np.zeros((S, A, S))
    sas[np.arange(S)[:, None], np.arange(A)[None, :], nxt] = 1.0
    return sas


def tables_of(world):
    """(compact tables for RefGridworld, dense sas) of a World."""
    tabs = world.compact()
    return tabs, sas_of(tabs['next'])


def walk_stores(tabs, n, seed, repeat=None):
    """``n`` stores along a seeded walk: rows [s, a, r, ns, 1 - end] — random steps, after a third
    of them the shortest way to the terminal state (so that the walk holds a terminal transition),
    random steps again from the start.  ``repeat`` = (position, times): the experience at that
    position is stored again that often."""
    rng = np.random.default_rng(seed)
    nxt, rew, term, starts = tabs['next'], tabs['reward'], tabs['terminal'], tabs['starts']
    S, A = nxt.shape

    def way_home(s):
        prev = {s: None}
        todo = [s]
        while todo:
            u = todo.pop(0)
            if term[u]:
                path = []
                while prev[u] is not None:
                    path.append(prev[u][1])
                    u = prev[u][0]
                return path[::-1]
            for a in range(A):
                v = int(nxt[u, a])
                if v not in prev:
                    prev[v] = (u, a)
                    todo.append(v)
        return []

    rows, s, plan = [], int(starts[0]), None
    while len(rows) < n:
        if plan is None and len(rows) >= n // 3:
            plan = way_home(s)
        a = plan.pop(0) if plan else int(rng.integers(A))
        ns = int(nxt[s, a])
        end = int(term[ns])
        rows.append([s, a, float(rew[ns]), ns, 1 - end])
        s = int(starts[0]) if end else ns
    if repeat:
        at, times = repeat
        rows[at + 1:at + 1] = [list(rows[at]) for _ in range(times)]
    return rows[:n]


def masked_actions(tabs):
    """An action mask with masked entries: the actions that leave a state where it is."""
    nxt = np.asarray(tabs['next']).astype(np.int64)
    mask = nxt != np.arange(nxt.shape[0])[:, None]
    mask[~mask.any(axis=1)] = True
    return mask


def script_for(stores, start, lengths=(1, 2, 7, 32), none_state=True):
    """The calls of one case: ['store', s, a, r, ns, t], ['set', name, value], ['mask'] (the
    update mask), ['update_sr'], ['replay', length, state or None, force_first or None, masked]."""
    half = len(stores) // 2
    ops = [['store'] + r for r in stores[:half]]
    ops += [['replay', n, start, None, False] for n in lengths]
    ops += [['store'] + r for r in stores[half:]]
    ops += [['replay', 7, start, None, True], ['replay', 7, start, 3, False]]
    if none_state:
        ops += [['replay', 7, None, None, False]]
    ops += [['set', 'allow_loops', True], ['replay', 32, start, None, False],
            ['set', 'allow_loops', False], ['set', 'equal_need', True], ['replay', 7, start, None, False],
            ['set', 'equal_need', False], ['set', 'equal_gain', True], ['replay', 7, start, None, True],
            ['set', 'equal_gain', False], ['set', 'ignore_barriers', False],
            ['replay', 7, start, None, False], ['set', 'ignore_barriers', True],
            ['set', 'min_gain_mode', 'other'], ['replay', 32, start, None, True],
            ['set', 'min_gain_mode', 'original'], ['mask'], ['replay', 32, start, None, True],
            ['replay', 2, stores[-1][0], stores[0][0], False]]
    return ops


class ScriptMemory:
    """The calls of a script on a memory with the reference's signatures.  ``pick``: the instance
    looked at of a device memory with several; ``index``: memory -> (memory stream index, policy
    stream index); ``need``: called with the op number before a replay with state None."""

    def __init__(self, mem, mask, pick=None, index=None, need=None, sr=None):
        self.mem, self.mask, self.pick, self.index, self.need, self.sr = mem, mask, pick, index, need, sr
        self.Q = np.zeros((mem.nb_states, mem.nb_actions))

    def _mine(self, x):
        return x if self.pick is None else x[self.pick]

    def run(self, ops) -> dict:
        rows, qs, idx, srs, needs = [], [], [], [], []
        mem = self.mem
        for k, op in enumerate(ops):
            if op[0] == 'set':
                assert op[1] in SWITCHES
                setattr(mem, op[1], op[2])
            elif op[0] == 'store':
                s, a, r, ns, t = op[1:]
                mem.store({'state': int(s), 'action': int(a), 'reward': float(r),
                           'next_state': int(ns), 'terminal': int(t)})
            elif op[0] == 'mask':
                mem.compute_update_mask()
            elif op[0] == 'update_sr':
                mem.update_sr()
            elif op[0] == 'replay':
                _, length, state, first, masked = op
                if self.sr is not None:
                    self.sr(len(srs))
                if state is None and self.need is not None:
                    self.need(len(needs))
                if state is None:
                    needs.append(np.array(self._mine_need(mem.compute_need(None))))
                ups, Q = mem.replay(self.Q, self.mask if masked else None, length, state, first)
                ups, Q = self._mine(ups), self._mine(Q)
                self.Q = np.array(Q.cpu().numpy() if hasattr(Q, 'cpu') else Q, dtype=np.float64)
                rows += [[k] + list(r) for r in rows_of(ups)]
                qs.append(self.Q.copy())
                srs.append(np.array(self._mine_sr(mem.SR), dtype=np.float64))
                idx.append(list(self.index(mem)))
        S = mem.nb_states
        return {'replayed': np.array(rows, dtype=np.float64).reshape(-1, 6), 'Q': np.array(qs),
                'index': np.array(idx, dtype=np.int64), 'SR': np.array(srs),
                'need': np.array(needs, dtype=np.float64).reshape(-1, S * mem.nb_actions),
                'T': np.array(self._mine_sr(mem.T), dtype=np.float64),
                'rewards': np.array(self._mine_sr(mem.rewards), dtype=np.float64),
                'states': np.array(self._mine_sr(mem.states)).astype(np.int16),
                'terminals': np.array(self._mine_sr(mem.terminals)).astype(np.int8),
                'update_mask': np.array(self._mine_sr(mem.update_mask)).astype(bool)}

    def _mine_sr(self, a):
        a = np.asarray(a)
        return a if self.pick is None else a[self.pick]

    def _mine_need(self, a):
        a = np.asarray(a)
        return a[self.pick] if (self.pick is not None and a.ndim == 2) else a


RECORD_KEYS = ('replayed', 'Q', 'index', 'T', 'rewards', 'states', 'terminals', 'update_mask')


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
