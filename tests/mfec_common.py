"""Helpers shared by the MFEC tests: a plain NumPy restatement of ``ActionBuffer``, ``QEC`` and of
``MFEC.train`` / ``test`` / ``predict_on_batch`` (agent/mfec.py:28-559 of the reference, call for
call), driven by ``TapeRNG``, and the recorder both the fixture generator and the tests use.

The observation of a tabular world is a function of the node, so the restatement works on a feature
table ``F[S, D]`` (row = ``process_observation`` of that node's observation) and its buffers hold
node ids.  What scikit-learn's ``KDTree`` contributes is restated as it is for a tree of ONE leaf
(up to 80 entries with the default ``leaf_size`` of 40): the reduced distance summed sequentially in
float64, every entry pushed in index order onto a fixed-size max-heap (sklearn/utils/_heap.pyx),
the heap then sorted by ``simultaneous_sort`` (sklearn/utils/_sorting.pyx), a quicksort that is not
stable.  Above 80 entries the real tree's answer among exact ties depends on how the tree was
split; there this restatement — the single-leaf rule continued — defines the semantics.

One deliberate difference: the reference stamps ``time.time()``; only the order of the stamps
matters, and here (and on the device, and in the recorder, which patches ``cobel.agent.mfec.time``)
the stamp is a per-agent counter that advances by one per training step.
"""
import numpy as np

from oracle.philox import STREAM_ENV, STREAM_POLICY, TapeRNG
from oracle.ref_loop import RefEpsilonGreedy, RefGridworld

RTOL, ATOL = 1e-04, 1e-06      # find_state's np.allclose (agent/mfec.py:76)


# -- what the tree computes ---------------------------------------------------------------------
def pair_tables(F):
    """(R, same): ``R[q, j]`` the reduced distance sum_d (F[q, d] - F[j, d])**2 accumulated
    sequentially in d with a separate multiply and add (sklearn's euclidean_rdist), ``same[q, j]``
    = np.allclose(F[j], F[q], rtol=1e-4, atol=1e-6) — stored entry j, query q; not symmetric."""
    F = np.asarray(F, dtype=np.float64)
    S, D = F.shape
    R = np.zeros((S, S))
    for d in range(D):
        t = F[:, None, d] - F[None, :, d]
        R = R + t * t
    same = np.zeros((S, S), dtype=bool)
    for q in range(S):
        for j in range(S):
            same[q, j] = np.allclose(F[j], F[q], rtol=RTOL, atol=ATOL)
    return R, same


def heap_push(vals, idx, val, i):
    """sklearn/utils/_heap.pyx: heap_push on a max-heap of fixed size."""
    size = len(vals)
    if val >= vals[0]:
        return
    vals[0], idx[0] = val, i
    cur = 0
    while True:
        left, right = 2 * cur + 1, 2 * cur + 2
        if left >= size:
            break
        elif right >= size:
            if vals[left] > val:
                swap = left
            else:
                break
        elif vals[left] >= vals[right]:
            if val < vals[left]:
                swap = left
            else:
                break
        else:
            if val < vals[right]:
                swap = right
            else:
                break
        vals[cur], idx[cur] = vals[swap], idx[swap]
        cur = swap
    vals[cur], idx[cur] = val, i


def simultaneous_sort(vals, idx, lo, size):
    """sklearn/utils/_sorting.pyx: simultaneous_sort on vals[lo:lo + size], idx alongside."""
    def swap(a, b):
        vals[lo + a], vals[lo + b] = vals[lo + b], vals[lo + a]
        idx[lo + a], idx[lo + b] = idx[lo + b], idx[lo + a]

    v = lambda a: vals[lo + a]      # noqa: E731
    if size <= 1:
        return
    if size == 2:
        if v(0) > v(1):
            swap(0, 1)
    elif size == 3:
        if v(0) > v(1):
            swap(0, 1)
        if v(1) > v(2):
            swap(1, 2)
            if v(0) > v(1):
                swap(0, 1)
    else:
        pivot = size // 2
        if v(0) > v(size - 1):
            swap(0, size - 1)
        if v(size - 1) > v(pivot):
            swap(size - 1, pivot)
            if v(0) > v(size - 1):
                swap(0, size - 1)
        pivot_val = v(size - 1)
        store = 0
        for i in range(size - 1):
            if v(i) < pivot_val:
                swap(i, store)
                store += 1
        swap(store, size - 1)
        pivot = store
        if pivot > 1:
            simultaneous_sort(vals, idx, lo, pivot)
        if pivot + 2 < size:
            simultaneous_sort(vals, idx, lo + pivot + 1, size - pivot - 1)


def tree_query(dist, k):
    """Indices ``KDTree.query(k)`` returns for the distances of the entries in index order (a
    single leaf): the pushes, then the sort."""
    vals, idx = [np.inf] * k, [0] * k
    for i, d in enumerate(dist):
        heap_push(vals, idx, float(d), i)
    simultaneous_sort(vals, idx, 0, k)
    return idx


# -- agent/mfec.py:28-237 -----------------------------------------------------------------------
class RefActionBuffer:
    def __init__(self, capacity):
        self.capacity = capacity
        self.ids, self.values, self.times = [], [], []

    def __len__(self):
        return len(self.ids)


class RefQEC:
    def __init__(self, F, nb_actions, capacity, k, tables=None):
        self.R, self.same = pair_tables(F) if tables is None else tables
        self.buffers = tuple(RefActionBuffer(capacity) for _ in range(nb_actions))
        self.k = k
        self.evicted = 0       # entries of a full buffer replaced by a newer one
        self.query = tree_query     # (tests/mfec_limits_common.py puts its faster, equal form here)

    def find_state(self, b, s):
        if not b.ids:
            return None
        i = self.query(self.R[s, b.ids], 1)[0]
        return i if self.same[s, b.ids[i]] else None

    def estimate(self, s, a):
        b = self.buffers[a]
        i = self.find_state(b, s)
        if i is not None:
            return b.values[i]
        if len(b) <= self.k:
            return 0.0
        value = 0.0
        for j in self.query(self.R[s, b.ids], self.k):
            value += b.values[j]
        return value / max(self.k, 1)

    def update(self, s, a, value, time):
        b = self.buffers[a]
        i = self.find_state(b, s)
        if i:       # (the reference's `if state_index:` — a hit at index 0 counts as a miss)
            b.values[i], b.times[i], b.ids[i] = max(b.values[i], value), max(b.times[i], time), s
        elif len(b) < b.capacity:
            b.ids.append(s), b.values.append(value), b.times.append(time)
        else:
            m = int(np.argmin(b.times))
            if time > b.times[m]:
                b.ids[m], b.values[m], b.times[m] = s, value, time
                self.evicted += 1


class RefMFEC:
    """agent/mfec.py:239-559 on a RefGridworld (the compact tables of a Topology)."""

    def __init__(self, F, nb_actions, policy, policy_test=None, capacity=2000, k=3, gamma=0.97,
                 tables=None):
        self.policy = policy
        self.policy_test = policy if policy_test is None else policy_test
        self.nb_actions, self.gamma = nb_actions, gamma
        self.Q = RefQEC(F, nb_actions, capacity, k, tables)
        self.clock = 0

    def retrieve_q(self, s):
        return np.array([self.Q.estimate(s, a) for a in range(self.nb_actions)])

    def _run(self, env, trials, steps, policy, learn, trace):
        for _ in range(trials):
            s, _ = env.reset()
            episode, ended = [], False
            for step in range(steps):
                q = self.retrieve_q(s)
                a = int(policy.select_action(q))
                ns, reward, end, _, _ = env.step(a)
                if learn:
                    self.clock += 1
                    episode.append([s, a, float(reward), float(self.clock)])
                if trace is not None:
                    trace['sar'].append((s, a, float(reward), float(end)))
                    trace['q'].append(q)
                s = ns
                if end:
                    ended = True
                    if learn:
                        r = 0.0
                        for e in episode[::-1]:
                            r = self.gamma * r + e[2]
                            e[2] = r
                        for es, ea, ev, et in episode:
                            self.Q.update(es, ea, ev, et)
                    break
            if trace is not None:
                trace['steps'].append(step)
                trace['ended'].append(ended)
                snapshot(trace, self.Q.buffers)

    def train(self, env, trials, steps=32, trace=None):
        self._run(env, trials, steps, self.policy, True, trace)

    def test(self, env, trials, steps=32, trace=None):
        self._run(env, trials, steps, self.policy_test, False, trace)

    def predict_on_batch(self, nodes):
        return np.array([[self.Q.estimate(int(s), a) for a in range(self.nb_actions)]
                         for s in nodes])


# -- records ------------------------------------------------------------------------------------
def new_trace():
    return {k: [] for k in ('sar', 'q', 'steps', 'ended', 'buf_len', 'buf_ids', 'buf_values',
                            'buf_times')}


def snapshot(trace, buffers, ids_of=None):
    """The buffers after a trial: lengths [A], then ids / values / times of all actions in turn."""
    trace['buf_len'].append([len(b) for b in buffers])
    for b in buffers:
        trace['buf_ids'] += list(b.ids) if ids_of is None else ids_of(b)
        trace['buf_values'] += list(b.values)
        trace['buf_times'] += list(b.times)


def pack(trace, n_actions):
    sar = np.array(trace['sar'], dtype=np.float64).reshape(-1, 4)
    return {'state': sar[:, 0].astype(np.int16), 'action': sar[:, 1].astype(np.int8),
            'reward': sar[:, 2], 'terminal': sar[:, 3].astype(np.int8),
            'q': np.array(trace['q'], dtype=np.float64).reshape(-1, n_actions),
            'steps': np.array(trace['steps'], dtype=np.int32),
            'ended': np.array(trace['ended'], dtype=bool),
            'buf_len': np.array(trace['buf_len'], dtype=np.int32).reshape(-1, n_actions),
            'buf_ids': np.array(trace['buf_ids'], dtype=np.int16),
            'buf_values': np.array(trace['buf_values'], dtype=np.float64),
            'buf_times': np.array(trace['buf_times'], dtype=np.float64)}


RECORD_KEYS = ('state', 'action', 'reward', 'terminal', 'q', 'steps', 'ended', 'buf_len', 'buf_ids',
               'buf_values', 'buf_times', 'index', 'predict')


def assert_same_record(got, want, prefix='', keys=RECORD_KEYS, what=''):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[prefix + k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError('%s %s differs first at %s: %r != %r'
                                 % (what, k, bad.tolist(), g[tuple(bad)], w[tuple(bad)]))


def tables_of(Z, name):
    """The compact tables a fixture case recorded."""
    return {k: Z['%s/tab_%s' % (name, k)] for k in ('next', 'reward', 'terminal', 'starts')}


def run_restatement(tab, F, cfg, seed, tables=None, query=None):
    """One recorded case on the restatement.  cfg: instance, trials, steps, capacity, k,
    test_trials, epsilon (x 1e6).  ``query``: a form of ``tree_query`` shown equal to it."""
    inst, trials, steps, capacity, k, test_trials, eps6 = [int(x) for x in cfg]
    env = RefGridworld(tab, TapeRNG(seed, inst, STREAM_ENV))
    A = np.asarray(tab['next']).shape[1]
    pol = RefEpsilonGreedy(eps6 / 1e6, TapeRNG(seed, inst, STREAM_POLICY))
    ag = RefMFEC(F, A, pol, capacity=capacity, k=k, tables=tables)
    if query is not None:
        ag.Q.query = query
    tr = new_trace()
    ag.train(env, trials, steps, trace=tr)
    if test_trials:
        ag.test(env, test_trials, steps, trace=tr)
    out = pack(tr, A)
    out['index'] = np.array([env.rng.index, pol.rng.index], dtype=np.int64)
    out['predict'] = ag.predict_on_batch(range(F.shape[0]))
    return out, ag
