"""What the MFEC tests at the top of the documented ranges share (tests/test_gpu_mfec_limits.py, the
host checks in tests/test_host_mfec.py, the second seed range of scripts/fuzz_mfec.py): faster forms
of the restatement's helpers, each shown equal to the plain one of tests/mfec_common.py on the CPU,
worlds and feature tables of up to 1 024 states and 8 actions, a restated agent started from a given
memory, and the device harness that keeps every array of a ``cobel_mfec_mem_t`` between sentinels.
"""
import ctypes as C

import numpy as np

import mfec_common as mc

PAD = 96                       # sentinel elements in front of and behind every framed array
SENTINEL, SENTINEL_I = -777.25, -7


# -- faster forms of the restatement ------------------------------------------------------------
def pair_tables(F):
    """``mfec_common.pair_tables`` without its S * S Python calls: ``R`` accumulated over d in order
    with a separate multiply and add, ``same`` from np.allclose's own inequality
    |stored - query| <= atol + rtol * |query| (finite inputs), one feature at a time."""
    F = np.asarray(F, dtype=np.float64)
    assert np.isfinite(F).all()
    S, D = F.shape
    R = np.zeros((S, S))
    same = np.ones((S, S), dtype=bool)
    for d in range(D):
        q, j = F[:, None, d], F[None, :, d]
        t = q - j
        R = R + t * t
        same &= np.abs(j - q) <= mc.ATOL + mc.RTOL * np.abs(q)
    return R, same


def tree_query(dist, k, block=128):
    """``mfec_common.tree_query`` that looks only at entries that can still enter the heap: of every
    ``block`` entries those below the root as it stood before the block (``heap_push`` rejects
    val >= root, and the root never grows), pushed in index order."""
    dist = np.asarray(dist, dtype=np.float64)
    vals, idx = [np.inf] * k, [0] * k
    for lo in range(0, len(dist), block):
        part = dist[lo:lo + block]
        for i in np.flatnonzero(part < vals[0]):
            mc.heap_push(vals, idx, float(part[i]), lo + int(i))
    mc.simultaneous_sort(vals, idx, 0, k)
    return idx


# -- worlds and features ---------------------------------------------------------------------------
def random_graph(S, A, seed, goals=1, n_starts=4):
    """Nodes (as a Topology takes them) of a random graph: every node has A neighbours drawn from
    all nodes, ``goals`` nodes are rewarded and terminal, ``n_starts`` others are the starts."""
    r = np.random.default_rng(seed)
    nbr = r.integers(0, S, (S, A))
    special = r.choice(S, goals + n_starts, replace=False)
    goal, starts = special[:goals], sorted(int(s) for s in special[goals:])
    terminal = np.zeros(S, dtype=bool)
    terminal[goal] = True
    return nodes_of(nbr, terminal.astype(np.float64), terminal), [str(s) for s in starts]


def line_graph(S):
    """A line of S nodes, two actions (left, right; the ends lead to themselves), the start at the
    left end and the only goal at the right end: a random walk needs about S * S steps."""
    s = np.arange(S)
    nbr = np.stack([np.maximum(s - 1, 0), np.minimum(s + 1, S - 1)], axis=1)
    terminal = s == S - 1
    return nodes_of(nbr, terminal.astype(np.float64), terminal), ['0']


def drawn_world(S, A, seed, goals=3):
    """(tables, sas) of a world whose rows are distributions: a random graph in which about half of
    the (state, action) pairs have two or three possible successors with random weights.  ``sas`` is
    the dense [S, A, S] tensor the restated environment draws from (also ``tables['sas']``);
    ``tables['next']`` the most likely successors, as cobel_world_create_n takes them."""
    r = np.random.default_rng(seed)
    sas = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            n = int(r.choice([1, 1, 2, 3]))
            succ = r.choice(S, n, replace=False)
            w = r.choice([0.1, 0.25, 0.5, 1.0, 2.0], n)
            sas[s, a, succ] = w
            sas[s, a] /= sas[s, a].sum()
    special = r.choice(S, goals + 3, replace=False)
    terminal = np.zeros(S, dtype=np.uint8)
    terminal[special[:goals]] = 1
    tab = {'next': np.argmax(sas, axis=2).astype(np.uint16), 'reward': terminal.astype(np.float64),
           'terminal': terminal, 'starts': np.sort(special[goals:]).astype(np.uint16), 'sas': sas}
    return tab, sas


def nodes_of(nbr, reward, terminal):
    S = len(nbr)
    return {str(i): {'id': str(i), 'pose': np.array([float(i % 32), float(i // 32), 0.0, 0.0, 0.0, 0.0]),
                     'neighbors': [str(int(j)) for j in nbr[i]], 'reward': float(reward[i]),
                     'terminal': bool(terminal[i])} for i in range(S)}


def tables_of(nodes, starts):
    """The compact tables of a Topology over these nodes, in the restatement's names."""
    ids = list(nodes)
    index = {key: i for i, key in enumerate(ids)}
    return {'next': np.array([[index[m] for m in nodes[key]['neighbors']] for key in ids], dtype=np.uint16),
            'reward': np.array([nodes[key]['reward'] for key in ids], dtype=np.float64),
            'terminal': np.array([bool(nodes[key]['terminal']) for key in ids]).astype(np.uint8),
            'starts': np.array([index[key] for key in starts]).astype(np.uint16)}


def tables(kind, S, seed=0):
    """(F, (R, same)) of a feature table.  One-hot rows: every term of a reduced distance is 0 or 1,
    their sum — two ones — exact in any order, so the tables are written down instead of summed
    over S features (tests/test_host_mfec.py shows the two agree)."""
    F = features(kind, S, seed)
    if kind == 'onehot':
        return F, (2.0 * (1.0 - np.eye(S)), np.eye(S, dtype=bool))
    return F, pair_tables(F)


def features(kind, S, seed=0):
    """Feature tables whose rows are all distinct and never allclose: ``random`` 16-d rows (no two
    distances tie), ``lattice`` the integer coordinates of a 32-wide grid (reduced distances are small
    integers: ties everywhere), ``onehot`` np.eye (every distinct pair at exactly 2)."""
    if kind == 'random':
        return np.random.default_rng(seed).random((S, 16))
    if kind == 'lattice':
        i = np.arange(S)
        return np.stack([i % 32, i // 32], axis=1).astype(np.float64)
    assert kind == 'onehot'
    return np.eye(S)


# -- memories ----------------------------------------------------------------------------------------
def built_buffer(S, length, rng, dups=None, times=None):
    """(ids, values, times) of a buffer the reference can produce: distinct nodes in random order,
    plus duplicates of its first node at later indices (QEC.update's ``if state_index:`` appends a
    revisited first node again) — as many as the length needs beyond ``S - 24`` distinct nodes, or
    ``dups``.  Stamps ascend unless given."""
    least = max(0, length - (S - 24))
    dups = least if dups is None else max(least, min(dups, length - 1))
    ids = rng.permutation(S)[:length - dups]
    if dups:
        at = np.sort(rng.choice(np.arange(1, length), dups, replace=False))
        full = np.full(length, ids[0])
        full[np.setdiff1d(np.arange(length), at)] = ids
        ids = full
    values = rng.random(length) * 2.0 - 0.5
    if times is None:
        times = np.arange(1, length + 1)
    return ids.astype(np.int64), values, np.broadcast_to(np.asarray(times, dtype=np.float64), (length,)).copy()


def load_memory(agent, memory, clock):
    """Start a restated agent (RefMFEC, or a bare RefQEC) from given buffers — per action ``ids``,
    ``values``, ``times`` — and a given clock."""
    Q = agent.Q if hasattr(agent, 'Q') else agent
    assert len(memory) == len(Q.buffers)
    for b, (ids, values, times) in zip(Q.buffers, memory):
        assert len(ids) == len(values) == len(times) <= b.capacity
        b.ids = [int(x) for x in ids]
        b.values = [float(x) for x in values]
        b.times = [float(x) for x in times]
    if hasattr(agent, 'Q'):
        agent.clock = int(clock)
    return agent


def count_updates(Q):
    """Wrap ``RefQEC.update`` so that it counts what each call did: ``inplace``, ``append``,
    ``replace``, ``refused`` (a full buffer whose oldest stamp is not older)."""
    counts = dict(inplace=0, append=0, replace=0, refused=0)
    plain = Q.update

    def update(s, a, value, time):
        b = Q.buffers[a]
        n, ev, i = len(b), Q.evicted, Q.find_state(b, s)
        plain(s, a, value, time)
        kind = 'inplace' if i else 'append' if len(b) > n else 'replace' if Q.evicted > ev else 'refused'
        counts[kind] += 1

    Q.update = update
    return counts


def restated(tab, F, tables, A, instance, seed, eps, capacity, k, gamma=0.97, memory=None, clock=0,
             drawn=False):
    """(agent, environment, policy) of the restatement for one instance, the fast query in place,
    started from ``memory``.  ``drawn``: ``tab`` holds dense ``sas`` rows and every step draws."""
    from oracle.philox import STREAM_ENV, STREAM_POLICY, TapeRNG
    from oracle.ref_loop import RefEpsilonGreedy, RefGridworld
    env = RefGridworld(tab, TapeRNG(seed, instance, STREAM_ENV, double_sub=1 if drawn else 0))
    pol = RefEpsilonGreedy(eps, TapeRNG(seed, instance, STREAM_POLICY))
    ag = mc.RefMFEC(F, A, pol, capacity=capacity, k=k, gamma=gamma, tables=tables)
    ag.Q.query = tree_query
    if memory is not None:
        load_memory(ag, memory, clock)
    return ag, env, pol


# -- the device ----------------------------------------------------------------------------------------
class Framed:
    """A device array in the middle of a buffer of sentinels."""

    def __init__(self, torch, shape, dtype, fill):
        count = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((count + 2 * PAD,), fill, dtype=dtype, device='cuda')
        self.view = self.buf[PAD:PAD + count].view(shape)

    def intact(self):
        return bool((self.buf[:PAD] == self.fill).all() and (self.buf[-PAD:] == self.fill).all())


def device_pairs(torch, F):
    """``cobel_mfec_pairs`` into framed tables."""
    from cobel_amd import _lib
    S, D = F.shape
    f = torch.as_tensor(np.ascontiguousarray(F, dtype=np.float64), device='cuda')
    r = Framed(torch, (S, S), torch.float64, SENTINEL)
    s = Framed(torch, (S, S), torch.uint8, 0xA5)
    _lib.check(_lib.lib().cobel_mfec_pairs(_lib.ptr(f), S, D, _lib.ptr(r.view), _lib.ptr(s.view), None))
    torch.cuda.synchronize()
    return r, s


def make_world(nxt, reward, terminal, starts, sas=None):
    """A world handle through the C ABI (cobel_world_create_n; with ``sas`` its rows become
    distributions through cobel_world_set_transitions).  cobel_world_destroy frees it."""
    from cobel_amd import _lib
    from cobel_amd.misc.gridworld_tools import transition_lists
    lib = _lib.lib()
    S, A = nxt.shape
    arrays = [np.ascontiguousarray(nxt, dtype=np.uint16), np.ascontiguousarray(reward, dtype=np.float32),
              np.ascontiguousarray(terminal, dtype=np.uint8), np.ascontiguousarray(starts, dtype=np.uint16),
              np.array([0, len(starts)], dtype=np.int32)]
    handle = C.c_void_p()
    _lib.check(lib.cobel_world_create_n(*[a.ctypes.data for a in arrays], S, 1, A, 0, C.byref(handle)))
    if sas is not None:
        off, st, cdf = transition_lists(sas)
        _lib.check(lib.cobel_world_set_transitions(handle, off.ctypes.data, st.ctypes.data,
                                                   cdf.ctypes.data, len(st)))
    return handle


class DeviceMFEC:
    """Caller-owned arrays of ``cobel_mfec_mem_t`` and ``cobel_mfec_run_t`` for N instances, every
    one framed by sentinels, and the calls through the C ABI."""

    def __init__(self, torch, F, N, A, capacity, k, steps=1, trace_cap=0, trial_cap=0):
        self.torch, self.N, self.A, self.cap, self.k, self.S = torch, N, A, capacity, k, F.shape[0]
        self.steps, self.trace_cap, self.trial_cap = steps, trace_cap, trial_cap
        from cobel_amd import _lib
        i32, f64 = torch.int32, torch.float64
        self.rdist, self.same = device_pairs(torch, F)
        self.f = {'ids': Framed(torch, (N, A, capacity), i32, SENTINEL_I),
                  'values': Framed(torch, (N, A, capacity), f64, SENTINEL),
                  'times': Framed(torch, (N, A, capacity), i32, SENTINEL_I),
                  'len': Framed(torch, (N, A), i32, SENTINEL_I),
                  'clock': Framed(torch, (N,), i32, SENTINEL_I),
                  'inst': Framed(torch, (N, _lib.I_WORDS), i32, SENTINEL_I),
                  'ep_sa': Framed(torch, (N, steps), i32, SENTINEL_I),
                  'ep_value': Framed(torch, (N, steps), f64, SENTINEL),
                  'trace': Framed(torch, (N, max(trace_cap, 1), 4 + A), f64, SENTINEL),
                  'trace_len': Framed(torch, (N,), i32, SENTINEL_I),
                  'lat_trace': Framed(torch, (N, max(trial_cap, 1)), i32, SENTINEL_I),
                  'rdist': self.rdist, 'same': self.same}
        self.t = {name: fr.view for name, fr in self.f.items()}
        for name in ('len', 'clock', 'inst', 'trace_len'):
            self.t[name].zero_()

    def load(self, i, memory, clock):
        torch = self.torch
        for a, (ids, values, times) in enumerate(memory):
            n = len(ids)
            self.t['ids'][i, a, :n] = torch.as_tensor(np.asarray(ids, dtype=np.int32), device='cuda')
            self.t['values'][i, a, :n] = torch.as_tensor(np.asarray(values, dtype=np.float64), device='cuda')
            self.t['times'][i, a, :n] = torch.as_tensor(np.asarray(times).astype(np.int32), device='cuda')
            self.t['len'][i, a] = n
        self.t['clock'][i] = int(clock)

    def mem(self):
        from cobel_amd import _lib
        m = _lib.MFECMem()
        for name in ('rdist', 'same', 'ids', 'values', 'times', 'len', 'clock'):
            setattr(m, name, _lib.ptr(self.t[name]))
        m.n, m.n_states, m.n_actions, m.capacity, m.k = self.N, self.S, self.A, self.cap, self.k
        return m

    def estimate(self, nodes):
        """cobel_mfec_estimate of ``nodes``: [N, B, A], its output framed."""
        from cobel_amd import _lib
        torch = self.torch
        nd = torch.as_tensor(np.asarray(nodes, dtype=np.int32), device='cuda')
        out = Framed(torch, (self.N, len(nodes), self.A), torch.float64, SENTINEL)
        m = self.mem()
        _lib.check(_lib.lib().cobel_mfec_estimate(C.byref(m), _lib.ptr(nd), len(nodes),
                                                  _lib.ptr(out.view), None))
        torch.cuda.synchronize()
        assert out.intact(), 'cobel_mfec_estimate wrote outside its output'
        return out.view.cpu().numpy()

    def set_counters(self, env_ctr, policy_ctr):
        from cobel_amd import _lib
        torch = self.torch
        self.t['inst'][:, _lib.I_CTR_ENV] = torch.as_tensor(np.asarray(env_ctr, dtype=np.int32), device='cuda')
        self.t['inst'][:, _lib.I_CTR_POLICY] = torch.as_tensor(np.asarray(policy_ctr, dtype=np.int32),
                                                               device='cuda')

    def run(self, world, trials_target, seed, instance_base, eps, gamma=0.97, learn=True):
        """cobel_mfec_run up to ``trials_target`` trials in all (the instances carry their own trial
        count between launches)."""
        from cobel_amd import _lib
        r, m = _lib.MFECRun(), self.mem()
        for name in ('inst', 'ep_sa', 'ep_value'):
            setattr(r, name, _lib.ptr(self.t[name]))
        if self.trace_cap:
            r.trace, r.trace_len, r.trace_cap = _lib.ptr(self.t['trace']), _lib.ptr(self.t['trace_len']), self.trace_cap
        if self.trial_cap:
            r.lat_trace, r.trial_cap = _lib.ptr(self.t['lat_trace']), self.trial_cap
        r.n, r.mon_stripes, r.instance_base, r.seed = self.N, 1, instance_base, seed
        r.flags = _lib.F_LEARN if learn else 0
        r.trials_target, r.steps_per_trial, r.step_budget = trials_target, self.steps, 0
        r.gamma, r.epsilon = gamma, eps
        self.t['inst'][:, _lib.I_FLAGS] = 0
        self.t['inst'][:, _lib.I_STEP] = 0
        _lib.check(_lib.lib().cobel_mfec_run(world, C.byref(m), C.byref(r), None))
        self.torch.cuda.synchronize()

    def host(self, name):
        return self.t[name].cpu().numpy()

    def check(self, refs, what=''):
        """The frames stand; ``len``, ``clock`` and the buffers equal the restated agents' (``refs[i]``
        a RefMFEC, a RefQEC, or None for an instance left alone); nothing behind ``len`` was written."""
        self.torch.cuda.synchronize()
        for name, fr in self.f.items():
            assert fr.intact(), (what, name, 'the frame is broken')
        lens, clock = self.host('len'), self.host('clock')
        got = {name: self.host(name) for name in ('ids', 'values', 'times')}
        for i, ref in enumerate(refs):
            if ref is None:
                continue
            Q = ref.Q if hasattr(ref, 'Q') else ref
            assert lens[i].tolist() == [len(b) for b in Q.buffers], (what, i, lens[i].tolist())
            if hasattr(ref, 'clock'):
                assert int(clock[i]) == ref.clock, (what, i, int(clock[i]), ref.clock)
            for a, b in enumerate(Q.buffers):
                n = len(b)
                for name, want, fill in (('ids', b.ids, SENTINEL_I), ('values', b.values, SENTINEL),
                                         ('times', b.times, SENTINEL_I)):
                    g = got[name][i, a]
                    if not np.array_equal(g[:n], np.asarray(want, dtype=g.dtype)):
                        at = int(np.flatnonzero(g[:n] != np.asarray(want, dtype=g.dtype))[0])
                        raise AssertionError('%s instance %d action %d %s differs first at %d: %r != %r'
                                             % (what, i, a, name, at, g[at], want[at]))
                    assert (g[n:] == fill).all(), (what, i, a, name, 'written behind len')

    def trace_rows(self, i):
        n = int(self.host('trace_len')[i])
        return self.host('trace')[i, :n]


def assert_trace(rows, tr, A, what=''):
    """The device's recorded steps (state, action, reward, end, q) against a restatement's trace."""
    want = np.concatenate([np.array(tr['sar'], dtype=np.float64).reshape(-1, 4),
                           np.array(tr['q'], dtype=np.float64).reshape(-1, A)], axis=1)
    assert rows.shape == want.shape, (what, rows.shape, want.shape)
    if not np.array_equal(rows, want):
        at = np.argwhere(rows != want)[0]
        raise AssertionError('%s step %d column %d: %r != %r'
                             % (what, at[0], at[1], rows[tuple(at)], want[tuple(at)]))
