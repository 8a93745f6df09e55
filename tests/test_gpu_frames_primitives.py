"""The stand-alone primitives of csrc/world.hip and csrc/general.hip — the raw stream access, the
row gather, the vectorised environment and epsilon-greedy — with every array inside a frame of
sentinels (tests/frames_common.py) AND against independent references: oracle/philox.py for the
streams, NumPy indexing for the gather and the environment, a NumPy restatement of
policy/greedy.py (``RefEpsilonGreedy`` of oracle/ref_loop.py) with ``searchsorted(side='right')``
for the selection.  All comparisons are exact."""
import numpy as np
import pytest
import torch

import frames_common as fc
from oracle import philox
from oracle.ref_loop import RefEpsilonGreedy

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEED = 0xC0BE1 | (0x1234 << 32)          # (both halves of the key in use)


def _L():
    from cobel_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# -- streams -----------------------------------------------------------------------------------------
def _indices(n, rng):
    """Draw counters: small ones, both parities and word positions, and 0xffffffff (wraps to 0)."""
    idx = rng.integers(0, 1000, n).astype(np.uint32)
    idx[0] = 0xffffffff
    idx[-1] = 0xffffffff if n > 1 else idx[-1]
    if n > 4:
        idx[1:5] = [0, 1, 2, 3]
    return idx


@pytest.mark.parametrize('advance', [0, 1])
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_rng_uniform(n, advance):
    L = _L()
    idx = _indices(n, np.random.default_rng(n))
    index = fc.frame(_dev(idx.view(np.int32)), fc.MARK)
    out = fc.frame(torch.full((n,), -3.0, dtype=torch.float64, device=DEV), fc.BIG)
    base, stream = 7, philox.STREAM_POLICY
    L.check(L.lib().cobel_rng_uniform(L.ptr(index.view), SEED, stream, base, L.ptr(out.view), n,
                                      advance, None))
    torch.cuda.synchronize()
    assert index.intact() and out.intact()
    want = philox.draw_double(SEED, base + np.arange(n), idx, 0, stream)
    assert np.array_equal(out.view.cpu().numpy(), want)
    assert np.array_equal(_u32(index.view), idx + np.uint32(advance))     # (uint32: wraps)


@pytest.mark.parametrize('advance', [0, 1])
@pytest.mark.parametrize('per', [1, 3, 50])
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_rng_bounded(n, per, advance):
    L = _L()
    idx = _indices(n, np.random.default_rng(n + per))
    base, stream = 11, philox.STREAM_MEMORY
    for bound in (1, 2, 1 << 31, (1 << 32) - 1):
        index = fc.frame(_dev(idx.view(np.int32)), fc.MARK)
        out = fc.frame(torch.full((n, per), -3, dtype=torch.int32, device=DEV), fc.MARK)
        L.check(L.lib().cobel_rng_bounded(L.ptr(index.view), SEED, stream, base, bound,
                                          L.ptr(out.view), n, per, advance, None))
        torch.cuda.synchronize()
        assert index.intact() and out.intact()
        want = philox.draw_bounded(SEED, (base + np.arange(n))[:, None], idx[:, None],
                                   np.arange(per)[None, :], stream, bound)
        assert np.array_equal(_u32(out.view).astype(np.int64), want), bound
        assert want.max() < bound and (bound < 3 or want.max() > bound // 2 or n * per < 8)
        assert np.array_equal(_u32(index.view), idx + np.uint32(advance))


@pytest.mark.parametrize('advance', [0, 1])
@pytest.mark.parametrize('per', [1, 3, 50])
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_rng_bounded_each(n, per, advance):
    """One bound per instance (DQN's memory sampling); a bound of 0 yields 0 and leaves that
    instance's counter alone."""
    L = _L()
    rng = np.random.default_rng(3 * n + per)
    idx = _indices(n, rng)
    bounds = rng.choice(np.array([0, 1, 2, 7, 1000, 1 << 31, (1 << 32) - 1], dtype=np.uint64),
                        n).astype(np.uint32)
    bounds[0] = 0 if n > 1 else 5
    bounds[-1] = (1 << 32) - 1
    base, stream = 5, philox.STREAM_MEMORY
    index = fc.frame(_dev(idx.view(np.int32)), fc.MARK)
    bnd = fc.frame(_dev(bounds.view(np.int32)), 1)
    out = fc.frame(torch.full((n, per), -3, dtype=torch.int32, device=DEV), fc.MARK)
    L.check(L.lib().cobel_rng_bounded_each(L.ptr(index.view), SEED, stream, base, L.ptr(bnd.view),
                                           L.ptr(out.view), n, per, advance, None))
    torch.cuda.synchronize()
    assert index.intact() and bnd.intact() and out.intact()
    want = philox.draw_bounded(SEED, (base + np.arange(n))[:, None], idx[:, None],
                               np.arange(per)[None, :], stream,
                               np.maximum(bounds, 1).astype(np.uint64)[:, None])
    want[bounds == 0] = 0
    assert np.array_equal(_u32(out.view).astype(np.int64), want)
    assert np.array_equal(_u32(index.view), idx + (bounds != 0).astype(np.uint32) * np.uint32(advance))
    assert np.array_equal(_u32(bnd.view), bounds)


# -- the row gather ----------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 40])
@pytest.mark.parametrize('width', [1, 6, 7])
def test_gather_rows(width, rows):
    """Topology observations: rows of a float64 table by index; -1 and ``rows`` give NaN rows."""
    L = _L()
    n = 257
    rng = np.random.default_rng(width * 100 + rows)
    tab = rng.standard_normal((rows, width))
    idx = rng.integers(0, rows, n).astype(np.int32)
    idx[[0, 100, n - 1]] = [-1, rows, rows - 1]
    idx[1], idx[2] = rows, -1
    table = fc.frame(_dev(tab), fc.BIG)
    index = fc.frame(_dev(idx), 0)
    out = fc.frame(torch.full((n, width), -3.0, dtype=torch.float64, device=DEV), fc.BIG)
    L.check(L.lib().cobel_gather_rows(L.ptr(table.view), L.ptr(index.view), L.ptr(out.view), n,
                                      width, rows, None))
    torch.cuda.synchronize()
    assert table.intact() and index.intact() and out.intact()
    ok = (idx >= 0) & (idx < rows)
    got = out.view.cpu().numpy()
    assert np.array_equal(got[ok], tab[idx[ok]])
    assert np.isnan(got[~ok]).all() and (~ok).sum() == 4
    assert np.array_equal(table.view.cpu().numpy(), tab)


# -- the vectorised environment ----------------------------------------------------------------------
def _worlds():
    from cobel_amd.interface import Gridworld, Topology
    from cobel_amd.misc.gridworld_tools import make_gridworld
    one = make_gridworld(5, 5, terminals=[12], goals=[12], starting_states=[24],
                         rewards=np.array([[12, 1.0], [23, 0.25], [1, -0.5]]))
    many = make_gridworld(20, 20, terminals=[210], goals=[210],
                          rewards=np.array([[210, 1.0], [398, 0.25], [1, -0.5]]),
                          starting_states=[s for s in range(400) if s != 210][:300])
    return {'a4_one_start': Gridworld(one, n_envs=1, seed=SEED),
            'a4_300_starts': Gridworld(many, n_envs=1, seed=SEED),
            'a6': Topology(fc.graph(40, 6, 6), None, n_envs=1, seed=SEED)}


@pytest.mark.parametrize('name', ['a4_one_start', 'a4_300_starts', 'a6'])
@pytest.mark.parametrize('n', [1, 257])
def test_env_step_reset_and_step_draw(name, n):
    """cobel_env_step / cobel_env_reset / cobel_env_step_draw on worlds of four and six actions,
    start lists of 1 and 300 (39 on the graph), reset masks, ``reward_out`` / ``done_out`` NULL."""
    L = _L()
    lib = L.lib()
    env = _worlds()[name]
    w = env.world
    nxt, rew, term = (np.asarray(w['next']), np.asarray(w['rewards'], dtype=np.float32),
                      np.asarray(w['terminals']).astype(np.uint8))
    starts = np.asarray(w['starting_states'])
    S, A = nxt.shape
    base = 9
    rng = np.random.default_rng(n + A)
    s0 = rng.integers(0, S, n).astype(np.int32)
    s0[-1] = S - 1
    act = rng.integers(0, A, n).astype(np.uint8)
    ctr0 = rng.integers(0, 50, n).astype(np.uint32)
    ctr0[0] = 0xffffffff
    for with_out in (True, False):
        for draw in (False, True):
            state = fc.frame(_dev(s0), 0)
            action = fc.frame(_dev(act), 0)
            reward = fc.frame(torch.full((n,), -3.0, device=DEV), fc.BIG)
            done = fc.frame(torch.full((n,), 7, dtype=torch.uint8, device=DEV), 0x5A)
            ctr = fc.frame(_dev(ctr0.view(np.int32)), fc.MARK)
            r_ptr, d_ptr = (L.ptr(reward.view), L.ptr(done.view)) if with_out else (None, None)
            if draw:     # (rows that are no distributions: steps as cobel_env_step, counters left alone)
                L.check(lib.cobel_env_step_draw(env.handle.ptr, L.ptr(state.view),
                                                L.ptr(action.view), r_ptr, d_ptr, L.ptr(ctr.view),
                                                SEED, n, base, None))
            else:
                L.check(lib.cobel_env_step(env.handle.ptr, L.ptr(state.view), L.ptr(action.view),
                                           r_ptr, d_ptr, n, base, None))
            torch.cuda.synchronize()
            for f in (state, action, reward, done, ctr):
                assert f.intact()
            ns = nxt[s0, act].astype(np.int32)
            assert np.array_equal(state.view.cpu().numpy(), ns)
            assert np.array_equal(_u32(ctr.view), ctr0)
            if with_out:
                assert np.array_equal(reward.view.cpu().numpy(), rew[ns])
                assert np.array_equal(done.view.cpu().numpy(), term[ns])
            else:
                assert bool((reward.view == -3.0).all()) and bool((done.view == 7).all())
    # reset: all instances, and those a mask names
    for masked in (False, True):
        m = (np.arange(n) % 3 != 1).astype(np.uint8) if masked else np.ones(n, dtype=np.uint8)
        state = fc.frame(_dev(s0), 0)
        ctr = fc.frame(_dev(ctr0.view(np.int32)), fc.MARK)
        mask = fc.frame(_dev(m), 1)
        L.check(lib.cobel_env_reset(env.handle.ptr, L.ptr(state.view),
                                    L.ptr(mask.view) if masked else None, L.ptr(ctr.view), SEED, n,
                                    base, None))
        torch.cuda.synchronize()
        assert state.intact() and ctr.intact() and mask.intact()
        k = philox.draw_bounded(SEED, base + np.arange(n), ctr0, 0, philox.STREAM_ENV, len(starts))
        want = np.where(m != 0, starts[k], s0).astype(np.int32)
        assert np.array_equal(state.view.cpu().numpy(), want)
        assert np.array_equal(_u32(ctr.view), ctr0 + (m != 0).astype(np.uint32))
        assert len(starts) == {'a4_one_start': 1, 'a4_300_starts': 300, 'a6': 38}[name]


@pytest.mark.parametrize('n', [1, 257])
@pytest.mark.parametrize('h,w', [(5, 5), (7, 9)])
def test_env_step_draw_on_distribution_rows(h, w, n):
    """cobel_env_step_draw on a slippery world (rows that are distributions): the successor is the
    first one whose cumulative probability exceeds the double of the env stream (sub-stream 1) at
    the instance's counter — ``searchsorted(side='right')`` on the reference's CDF —, rewards and
    ends belong to the state entered, every counter advances by one; state, action, reward, done
    and the counters framed, ``reward_out`` / ``done_out`` also NULL, counters at 0xffffffff."""
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_gridworld
    L = _L()
    lib = L.lib()
    S = h * w
    world = make_gridworld(h, w, terminals=[S // 2], goals=[S // 2], starting_states=[S - 1],
                           rewards=np.array([[S // 2, 1.0], [S - 2, 0.25], [1, -0.5]]))
    sas = np.array(world['sas'])
    sas = 0.75 * sas + 0.125 * sas[:, [1, 2, 3, 0]] + 0.125 * sas[:, [3, 0, 1, 2]]
    world['sas'], world['deterministic'] = sas, False
    env = Gridworld(world, n_envs=1, seed=SEED)
    assert env.handle.stochastic
    rew = np.asarray(world['rewards'], dtype=np.float32)
    term = np.asarray(world['terminals']).astype(np.uint8)
    base = 9
    rng = np.random.default_rng(S + n)
    s0 = rng.integers(0, S, n).astype(np.int32)
    s0[-1] = S - 1
    act = rng.integers(0, 4, n).astype(np.uint8)
    ctr0 = rng.integers(0, 50, n).astype(np.uint32)
    ctr0[0] = 0xffffffff
    u = philox.draw_double(SEED, base + np.arange(n), ctr0, 1, philox.STREAM_ENV)
    cdf = np.cumsum(sas[s0, act], axis=1)
    cdf /= cdf[:, -1:]
    ns = (cdf <= u[:, None]).sum(axis=1).astype(np.int32)
    if n > 1:
        assert (ns != np.asarray(world['next'])[s0, act]).any(), 'no instance slipped'
    for with_out in (True, False):
        state = fc.frame(_dev(s0), 0)
        action = fc.frame(_dev(act), 0)
        reward = fc.frame(torch.full((n,), -3.0, device=DEV), fc.BIG)
        done = fc.frame(torch.full((n,), 7, dtype=torch.uint8, device=DEV), 0x5A)
        ctr = fc.frame(_dev(ctr0.view(np.int32)), fc.MARK)
        r_ptr, d_ptr = (L.ptr(reward.view), L.ptr(done.view)) if with_out else (None, None)
        L.check(lib.cobel_env_step_draw(env.handle.ptr, L.ptr(state.view), L.ptr(action.view),
                                        r_ptr, d_ptr, L.ptr(ctr.view), SEED, n, base, None))
        torch.cuda.synchronize()
        for f in (state, action, reward, done, ctr):
            assert f.intact()
        assert np.array_equal(state.view.cpu().numpy(), ns)
        assert np.array_equal(_u32(ctr.view), ctr0 + np.uint32(1))        # (uint32: wraps to 0)
        assert np.array_equal(action.view.cpu().numpy(), act)
        if with_out:
            assert np.array_equal(reward.view.cpu().numpy(), rew[ns])
            assert np.array_equal(done.view.cpu().numpy(), term[ns])
        else:
            assert bool((reward.view == -3.0).all()) and bool((done.view == 7).all())


# -- epsilon-greedy ----------------------------------------------------------------------------------
N_ROWS = 257


def _value_rows(A, rng):
    """Rows with ties of every count (1 .. A), -0.0 against +0.0, and all values -inf."""
    rows = []
    for k in range(1, A + 1):
        v = rng.integers(-3, 3, A).astype(np.float64) - 10.0
        v[rng.permutation(A)[:k]] = 2.5
        rows.append(v)
    z = np.zeros(A)
    z[::2] = -0.0
    rows.append(z)                                   # every action ties: -0.0 == +0.0
    z = np.full(A, -1.0)
    z[0], z[-1] = 0.0, -0.0
    rows.append(z)
    rows.append(np.full(A, -np.inf))
    return rows


def _masks(A, rng):
    """None, all bits, one bit (first, last), a random set."""
    full = (1 << A) - 1
    out = [None, full, 1, 1 << (A - 1)]
    for _ in range(3):
        m = int(rng.integers(1, full + 1)) if A < 32 else int(rng.integers(1, 1 << 32))
        out.append(m)
    return out


def _cases(A, eps, rng):
    """The whole universe of (values, mask bits or None, u): every value row under every mask, u at
    0, at 1 - 2^-53, on every entry of the reference's CDF and one ulp below it."""
    ref = RefEpsilonGreedy(eps, None)
    rows = []
    for v in _value_rows(A, rng):
        for m in _masks(A, rng):
            mb = None if m is None else np.array([(m >> a) & 1 for a in range(A)], dtype=bool)
            cdf = np.cumsum(ref.get_action_probs(v, mb))
            cdf /= cdf[-1]
            us = [0.0, 1.0 - 2.0 ** -53]
            for c in cdf:
                us += [c, np.nextafter(c, -1.0)]
            rows += [(v, m, u) for u in sorted({u for u in us if 0.0 <= u < 1.0})]
    return rows


def _reference(rows, A, eps):
    ref = RefEpsilonGreedy(eps, None)
    act = np.zeros(len(rows), dtype=np.uint8)
    probs = np.zeros((len(rows), A))
    for i, (v, m, u) in enumerate(rows):
        mb = None if m is None else np.array([(m >> a) & 1 for a in range(A)], dtype=bool)
        p = ref.get_action_probs(v, mb)
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        act[i] = int(cdf.searchsorted(u, side='right'))
        probs[i] = p
    return act, probs


@pytest.mark.parametrize('f64', [False, True])
@pytest.mark.parametrize('eps', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('A', [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32])
def test_eps_greedy_n(A, eps, f64):
    """cobel_eps_greedy_n / _n_f64 (and, at four actions, cobel_eps_greedy / _f64) against the
    restatement: actions and ``probs_out`` exact; byte masks up to eight actions, word masks
    beyond; masked and unmasked rows in separate launches (a mask pointer serves all rows).  The
    whole universe of ``_cases`` runs, 257 rows per launch (A = 32: about 8 000 rows, 32 launches)."""
    L = _L()
    lib = L.lib()
    rng = np.random.default_rng(1000 * A + int(eps * 10) + f64)
    rows = _cases(A, eps, rng)
    # nothing of what the cases are about is left to chance: ties of every count, the signed zeros,
    # the all -inf row, masks of one bit and of all bits — and every row of the universe is run
    plain_rows = [r for r in rows if r[1] is None]
    assert {int((r[0] == r[0].max()).sum()) for r in plain_rows} == set(range(1, A + 1))
    assert any(np.isneginf(r[0]).all() for r in rows)
    assert any(np.signbit(r[0]).any() and not r[0].any() for r in rows)
    assert {1, 1 << (A - 1), (1 << A) - 1} <= {r[1] for r in rows}
    for masked in (False, True):
        universe = [r for r in rows if (r[1] is not None) == masked]
        chunks = -(-len(universe) // N_ROWS)
        for c in range(chunks):
            # (257 rows per launch; the last chunk is filled up from the start of the universe)
            sel = (universe[c * N_ROWS:] + universe)[:N_ROWS]
            _eps_greedy_chunk(L, lib, sel, A, eps, f64, masked)


def _eps_greedy_chunk(L, lib, sel, A, eps, f64, masked):
    n = len(sel)
    vals = np.stack([r[0] for r in sel]).astype(np.float64 if f64 else np.float32)
    us = np.array([r[2] for r in sel])
    want_a, want_p = _reference([(vals[i].astype(np.float64), sel[i][1], us[i]) for i in range(n)],
                                A, eps)
    entries = [(lib.cobel_eps_greedy_n_f64 if f64 else lib.cobel_eps_greedy_n, True)]
    if A == 4:
        entries.append((lib.cobel_eps_greedy_f64 if f64 else lib.cobel_eps_greedy, False))
    for entry, takes_a in entries:
        values = fc.frame(_dev(vals), fc.BIG)
        u = fc.frame(_dev(us), 0.0)
        act = fc.frame(torch.full((n,), 0x77, dtype=torch.uint8, device=DEV), 0x5A)
        probs = fc.frame(torch.full((n, A), -3.0, dtype=torch.float64, device=DEV), fc.BIG)
        mask = None
        if masked:
            bits = np.array([r[1] for r in sel], dtype=np.uint64)
            mb = bits.astype(np.uint8) if A <= 8 else bits.astype(np.uint32).view(np.int32)
            mask = fc.frame(_dev(mb), 1)
        args = [L.ptr(values.view), None if mask is None else L.ptr(mask.view), L.ptr(u.view),
                eps, L.ptr(act.view), L.ptr(probs.view), n] + ([A] if takes_a else []) + [None]
        L.check(entry(*args))
        torch.cuda.synchronize()
        for f in (values, u, act, probs) + ((mask,) if masked else ()):
            assert f.intact()
        got_a, got_p = act.view.cpu().numpy(), probs.view.cpu().numpy()
        assert fc.same_bits(got_p, want_p), (A, eps, f64, masked,
                                             np.flatnonzero((got_p != want_p).any(axis=1))[:5])
        bad = np.flatnonzero(got_a != want_a)
        assert bad.size == 0, (A, eps, f64, masked,
                               [(sel[i][0], sel[i][1], float(us[i]), int(got_a[i]), int(want_a[i]))
                                for i in bad[:3]])
        # probs_out NULL: the same actions
        act2 = fc.frame(torch.full((n,), 0x77, dtype=torch.uint8, device=DEV), 0x5A)
        args[4], args[5] = L.ptr(act2.view), None
        L.check(entry(*args))
        torch.cuda.synchronize()
        assert act2.intact() and torch.equal(act2.view, act.view)
