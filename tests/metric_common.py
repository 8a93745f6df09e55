"""The NumPy restatement of the device metrics (csrc/metric.hip, ``SR`` / ``DR`` with
``compute='device'``): the specification the kernels equal bit for bit, the worlds the tests run
on, and the fillers of the C calls' arguments.

Everything is float64 with one rounding per operation.

``init_L``         L = I - gamma T from the compact table: T[s][c] = count / 4 (exact), 1.0 - gamma t
                   on the diagonal and 0.0 - gamma t elsewhere
``gauss_jordan``   in place, pivots ascending, no pivoting: the pivot row scaled by 1 / pivot (the
                   pivot's own place takes 1 / pivot), every other element M - col[r] * row[c]
                   (0 - col[r] * row[k] in column k)
``pivoted_inverse`` the same steps after a row swap that brings the largest magnitude of the column
                   (lowest row on ties) to the pivot; the swaps are undone as column swaps in
                   reverse order
``woodbury``       delta = (I - gamma T_new)[J] - (I - gamma T_default)[J]; A = I_k + delta D0[:, J];
                   alpha = A^-1; X = delta D0, Y = D0[:, J] alpha, B = Y X, D = D0 - B; every sum
                   starts at 0.0 and adds its terms in ascending index order, the terms of delta that
                   are exactly zero left out
The same functions run in ``np.longdouble`` (80 bits on x86) give the solutions accuracy is
measured against."""
import ctypes as C

import numpy as np

EPS = 2.0 ** -53
MAX_STATES, MAX_RANK = 16383, 128
# e_restatement <= F * max(e_host, 2^-53 max|D|): twice the worst ratio measured over CASES
# (docs/MEASUREMENTS.md, "Device metrics"; tests/test_host_metric.py prints the table)
F = 15.4


# -- worlds ------------------------------------------------------------------------------------------
def open_table(width, height):
    """Compact successor table of the open field, moves clamped at the border (left, up, right,
    down: the order of DR.build_default_transition_matrix)."""
    n = width * height
    rows, cols = np.divmod(np.arange(n), width)
    nxt = np.stack([rows * width + np.maximum(0, cols - 1),
                    np.maximum(0, rows - 1) * width + cols,
                    rows * width + np.minimum(width - 1, cols + 1),
                    np.minimum(height - 1, rows + 1) * width + cols], axis=1)
    return np.ascontiguousarray(nxt, dtype=np.int32)


def with_walls(width, height, walls):
    """``walls``: pairs of neighbouring states; the move between them is blocked both ways (the
    agent stays).  Returns (next [S, 4] int32, invalid_transitions as a list of (s, s') tuples)."""
    nxt = open_table(width, height).copy()
    invalid = []
    for a, b in walls:
        for s, t in ((a, b), (b, a)):
            hit = (nxt[s] == t) & (s != t)
            assert hit.any(), 'states %d and %d are no neighbours' % (s, t)
            nxt[s, hit] = s
            if (s, t) not in invalid:
                invalid.append((int(s), int(t)))
    return nxt, invalid


def neighbours(width, height):
    out = []
    for s in range(width * height):
        r, c = divmod(s, width)
        if c + 1 < width:
            out.append((s, s + 1))
        if r + 1 < height:
            out.append((s, s + width))
    return out


def maze(width, height, p, seed, isolated=(), max_walls=None):
    """Each pair of neighbours is walled off with probability ``p``; the cells in ``isolated`` are
    walled off on every side.  ``max_walls`` keeps the first that many drawn walls."""
    rng = np.random.default_rng(seed)
    pairs = neighbours(width, height)
    drawn = [pr for pr in pairs if rng.random() < p]
    if max_walls is not None:
        drawn = drawn[:max_walls]
    walls = list(drawn)
    for cell in isolated:
        walls += [pr for pr in pairs if cell in pr and pr not in walls]
    return with_walls(width, height, walls)


def affected(invalid):
    """J: np.unique of the first members of ``invalid_transitions`` (metrics.py:238)."""
    if len(invalid) == 0:
        return np.zeros(0, dtype=np.int32)
    return np.unique(np.array(invalid)[:, 0]).astype(np.int32)


def world_of_rank(width, height, k, seed=0):
    """A world whose J has exactly ``k`` states: walls between disjoint pairs of neighbours (two
    states each); an odd k takes one chain of three states (two walls sharing the middle one), and
    k = 1 one move blocked in one direction only."""
    assert 0 <= k <= width * height
    rng = np.random.default_rng(seed)
    pairs = neighbours(width, height)
    order = rng.permutation(len(pairs))
    used, walls = set(), []
    if k % 2 == 1:
        if k == 1:
            nxt = open_table(width, height).copy()
            s = width + 1
            nxt[s, 2] = s
            return nxt, [(s, s + 1)]
        s = width + 1
        walls += [(s, s + 1), (s + 1, s + 2)]
        used |= {s, s + 1, s + 2}
    for q in order:
        if len(used) >= k:
            break
        a, b = pairs[q]
        if a in used or b in used:
            continue
        walls.append((a, b))
        used |= {a, b}
    assert len(used) == k, 'the grid has no room for rank %d' % k
    nxt, invalid = with_walls(width, height, walls)
    assert len(affected(invalid)) == k
    return nxt, invalid


# -- the restatement -----------------------------------------------------------------------------------
def transition_matrix(nxt, dtype=np.float64):
    nxt = np.asarray(nxt)
    n = nxt.shape[0]
    cnt = np.zeros((n, n), dtype=dtype)
    for a in range(4):
        np.add.at(cnt, (np.arange(n), nxt[:, a].astype(np.int64)), 1)
    return cnt * dtype(0.25)


def init_L(nxt, gamma, dtype=np.float64):
    T = transition_matrix(nxt, dtype)
    return np.eye(T.shape[0], dtype=dtype) - dtype(gamma) * T


def gauss_jordan(L):
    M = np.array(L, copy=True)
    one = M.dtype.type(1.0)
    for k in range(M.shape[0]):
        inv = one / M[k, k]
        col = M[:, k].copy()
        row = M[k, :].copy()
        row[k] = one
        row = row * inv
        M[:, k] = 0.0
        M = M - np.outer(col, row)
        M[k, :] = row
    return M


def pivoted_inverse(A):
    M = np.array(A, copy=True)
    k = M.shape[0]
    one = M.dtype.type(1.0)
    piv = np.zeros(k, dtype=np.int64)
    for kk in range(k):
        p = kk + int(np.argmax(np.abs(M[kk:, kk])))        # (argmax: the first of equal maxima)
        piv[kk] = p
        if p != kk:
            M[[kk, p], :] = M[[p, kk], :]
        inv = one / M[kk, kk]
        col = M[:, kk].copy()
        row = M[kk, :].copy()
        row[kk] = one
        row = row * inv
        M[:, kk] = 0.0
        M = M - np.outer(col, row)
        M[kk, :] = row
    for kk in range(k - 1, -1, -1):
        p = piv[kk]
        if p != kk:
            M[:, [kk, p]] = M[:, [p, kk]]
    return M


def sr_ref(nxt, gamma, dtype=np.float64):
    return gauss_jordan(init_L(nxt, gamma, dtype))


def delta_rows(nxt, nxt_default, J, gamma, dtype=np.float64):
    J = np.asarray(J, dtype=np.int64)
    return init_L(nxt, gamma, dtype)[J] - init_L(nxt_default, gamma, dtype)[J]


def sparse_times(delta, M):
    """delta M with the sums from 0.0 over the non-zero terms of a row of delta, ascending."""
    out = np.zeros((delta.shape[0], M.shape[1]), dtype=M.dtype)
    for i in range(delta.shape[0]):
        acc = np.zeros(M.shape[1], dtype=M.dtype)
        for c in np.flatnonzero(delta[i]):
            acc = acc + delta[i, c] * M[c]
        out[i] = acc
    return out


def woodbury(D0, nxt, nxt_default, J, gamma):
    J = np.asarray(J, dtype=np.int64)
    k = len(J)
    if k == 0:
        return D0.copy()
    dtype = D0.dtype.type
    delta = delta_rows(nxt, nxt_default, J, gamma, dtype)
    cols = D0[:, J]
    A = np.eye(k, dtype=dtype) + sparse_times(delta, cols)
    alpha = pivoted_inverse(A)
    X = sparse_times(delta, D0)
    Y = np.zeros(cols.shape, dtype=dtype)
    for i in range(k):
        Y = Y + np.outer(cols[:, i], alpha[i])
    B = np.zeros(D0.shape, dtype=dtype)
    for i in range(k):
        B = B + np.outer(Y[:, i], X[i])
    return D0 - B


def dr_ref(width, height, nxt, invalid, gamma, D0=None):
    default = open_table(width, height)
    if D0 is None:
        D0 = sr_ref(default, gamma)
    return woodbury(D0, nxt, default, affected(invalid), gamma)


def exact(nxt, gamma):
    """inv(I - gamma T) by the same elimination in 80 bits (np.longdouble; callers round)."""
    return gauss_jordan(init_L(nxt, gamma, np.longdouble))


def refined(nxt, gamma, start, rounds=2):
    """The 80-bit solution where the 80-bit elimination is not affordable (S^3 longdouble operations):
    iterative refinement of the float64 inverse ``start``, X <- X + start (I - L X), the residual
    in np.longdouble straight from the compact table (5 S^2 operations: L has at most five entries
    per row, gamma t is exact in 64 bits), the correction — of the size of start's error — by a
    float64 product.  Each round divides the error by about 2^53 / cond until the residual's own
    rounding, 2^-64 |L| |X|, is what is left; tests/test_host_metric.py checks it against ``exact``."""
    nxt = np.asarray(nxt, dtype=np.int64)
    g = np.longdouble(gamma) * np.longdouble(0.25)
    X = np.asarray(start, dtype=np.longdouble)
    eye = np.eye(nxt.shape[0], dtype=np.longdouble)
    for _ in range(rounds):
        TX = X[nxt[:, 0]] + X[nxt[:, 1]] + X[nxt[:, 2]] + X[nxt[:, 3]]
        R = eye - (X - g * TX)
        X = X + np.matmul(start, R.astype(np.float64)).astype(np.longdouble)
    return X


# -- the accuracy cases --------------------------------------------------------------------------------
# name -> (width, height, wall probability, seed, gamma, isolated cells)
CASES = {
    'open_5x5_g0.9': (5, 5, 0.0, 1, 0.9, ()),
    'maze_6x7_g0.9': (6, 7, 0.1, 2, 0.9, ()),
    'maze_10x10_g0.95': (10, 10, 0.2, 3, 0.95, ()),
    'maze_16x16_g0.99': (16, 16, 0.1, 4, 0.99, ()),
    'maze_20x13_g0.999': (20, 13, 0.1, 5, 0.999, ()),
    'isolated_12x12_g0.999': (12, 12, 0.05, 6, 0.999, (0, 77)),
}


def case_world(name):
    w, h, p, seed, gamma, isolated = CASES[name]
    nxt, invalid = maze(w, h, p, seed, isolated)
    return w, h, nxt, invalid, gamma


def errors(D_dev, D_host, D80):
    """(e_host, e_dev, floor) of bound (b)."""
    ex = np.asarray(D80, dtype=np.longdouble)
    e_host = float(np.abs(D_host.astype(np.longdouble) - ex).max())
    e_dev = float(np.abs(D_dev.astype(np.longdouble) - ex).max())
    return e_host, e_dev, EPS * float(np.abs(ex).max())


# -- the C calls -----------------------------------------------------------------------------------------
def j_arrays(Js, max_rank=None):
    """Host arrays of cobel_metric_dr: J [W][max_rank] int32 (rows padded with -1), rank [W]."""
    rank = np.array([len(j) for j in Js], dtype=np.int32)
    kmax = int(rank.max()) if max_rank is None else int(max_rank)
    J = np.full((len(Js), max(kmax, 1)), -1, dtype=np.int32)[:, :kmax]
    J = np.ascontiguousarray(J)
    for w, j in enumerate(Js):
        J[w, :len(j)] = j
    return J, rank, kmax


def plan(n_states, rank):
    from cobel_amd import _lib
    out = (C.c_int64 * 4)()
    rc = _lib.lib().cobel_metric_plan(n_states, rank, C.byref(out))
    return rc, list(out)


def work_bytes(n_worlds, n_states, max_rank):
    rc, out = plan(n_states, max_rank)
    assert rc == 0
    return (4 * n_worlds * (1 + max_rank) + 15) // 16 * 16 + n_worlds * out[3]


def pivot_swaps(A):
    """Rows ``pivoted_inverse`` swaps on A."""
    M, n = np.array(A, copy=True), 0
    for kk in range(M.shape[0]):
        p = kk + int(np.argmax(np.abs(M[kk:, kk])))
        if p != kk:
            M[[kk, p], :] = M[[p, kk], :]
            n += 1
        col, row = M[:, kk].copy(), M[kk, :].copy()
        row[kk] = 1.0
        row = row * (1.0 / M[kk, kk])
        M[:, kk] = 0.0
        M = M - np.outer(col, row)
        M[kk, :] = row
    return n


def woodbury_block(width, height, nxt, invalid, gamma):
    """A = I_k + delta D0[:, J] of a world."""
    default = open_table(width, height)
    J = affected(invalid).astype(np.int64)
    D0 = sr_ref(default, gamma)
    return np.eye(len(J)) + sparse_times(delta_rows(nxt, default, J, gamma), D0[:, J])


# -- the device calls (GPU tests) --------------------------------------------------------------------------
SHAPES = {1: (1, 1), 2: (2, 1), 25: (5, 5), 31: (31, 1), 32: (8, 4), 33: (11, 3), 63: (9, 7),
          64: (8, 8), 65: (13, 5), 96: (12, 8), 129: (43, 3), 272: (17, 16)}


def sr_worlds(S):
    """Three worlds of S states: the open field, a maze, a maze with an isolated cell."""
    w, h = SHAPES[S]
    iso = (w * h // 2,) if S >= 25 else ()
    return [open_table(w, h), maze(w, h, 0.15, 100 + S)[0], maze(w, h, 0.1, 200 + S, iso)[0]]


def device_sr(tabs, gamma, frames=None, out=None):
    """cobel_metric_sr on a stack of tables [W][S][4]; ``frames``: a frames_common.Frames that
    takes the inputs and the output."""
    import torch
    from cobel_amd import _lib
    from frames_common import BIG
    tabs = np.ascontiguousarray(tabs, dtype=np.int32)
    W, S = tabs.shape[0], tabs.shape[1]
    dev = torch.device('cuda', torch.cuda.current_device())
    nxt = torch.as_tensor(tabs, device=dev)
    D = torch.full((W, S, S), BIG, dtype=torch.float64, device=dev) if out is None else out
    if frames is not None:
        nxt = frames.add('next', nxt, 0)
        D = frames.add('D', D, BIG)
    _lib.check(_lib.lib().cobel_metric_sr(_lib.ptr(nxt), W, S, float(gamma), _lib.ptr(D),
                                          _lib.current_stream(dev)))
    torch.cuda.synchronize()
    return D


def device_dr(D0, tabs, default, Js, gamma, frames=None, max_rank=None, check=True):
    """cobel_metric_dr; returns (rc, D, work)."""
    import torch
    from cobel_amd import _lib
    from frames_common import BIG, MARK
    tabs = np.ascontiguousarray(tabs, dtype=np.int32)
    W, S = tabs.shape[0], tabs.shape[1]
    J, rank, kmax = j_arrays(Js, max_rank)
    dev = torch.device('cuda', torch.cuda.current_device())
    nxt = torch.as_tensor(tabs, device=dev)
    dflt = torch.as_tensor(np.ascontiguousarray(default, dtype=np.int32), device=dev)
    D0 = torch.as_tensor(D0, device=dev).contiguous()
    D = torch.full((W, S, S), BIG, dtype=torch.float64, device=dev)
    nbytes = _lib.metric_work_bytes(W, S, min(kmax, MAX_RANK))
    work = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    if frames is not None:
        nxt = frames.add('next', nxt, 0)
        dflt = frames.add('next_default', dflt, 0)
        D0 = frames.add('D0', D0, BIG)
        D = frames.add('D', D, BIG)
        work = frames.add('work', work, MARK & 0xFF)
    rc = _lib.lib().cobel_metric_dr(_lib.ptr(D0), _lib.ptr(nxt), _lib.ptr(dflt),
                                    J.ctypes.data if kmax else None, rank.ctypes.data, kmax, W, S,
                                    float(gamma), _lib.ptr(D), _lib.ptr(work), nbytes,
                                    _lib.current_stream(dev))
    torch.cuda.synchronize()
    if check:
        _lib.check(rc)
    return rc, D, work
