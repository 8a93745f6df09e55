"""Helpers of the tests of ``cobel_pma_stationary`` (csrc/pma_need.hip): the kernel restated in
NumPy in the device's operation order, the same system solved in ``np.longdouble``, and the cases
the fixture tests/golden/pma_need.npz holds.

The quantity: ``PMAMemory.compute_need(None)`` (memory/pma.py:403-408) is |v| for the unit-2-norm
left eigenvector v of T for the eigenvalue 1.  T is row-stochastic, so v is the stationary
distribution pi of T scaled to 2-norm 1, and pi solves

    (I - T + (1/S) 1 1^T)^T x = (1/S) 1

(pi (I - T) = 0 and pi 1 = 1 give pi (I - T + (1/S) 1 1^T) = (1/S) 1^T; the matrix is regular
whenever the eigenvalue 1 of T is simple).
"""
import numpy as np

import pma_common as pc

WORLDS = {
    'small_3x4': pc.small_world,                         # S = 12, less than a wavefront
    'demo_5x5': pc.demo_world,                           # 25
    'seeded_11x11': lambda: pc.seeded_world(11, 11, 5),  # 121, ragged
    'seeded_8x16': lambda: pc.seeded_world(8, 16, 3),    # 128, the limit
}
STORES = (0, 10, 60, 400, 3000)
WALK_SEED = 7
GAP_CONDITIONED = 1e-4
# where the second-smallest |eig - 1| is below GAP_CONDITIONED (asserted against the fixture's gaps)
ILL_CONDITIONED = (('demo_5x5', 60), ('demo_5x5', 3000))
CASES = tuple((w, n) for w in WORLDS for n in STORES)
EPS = 2.0 ** -53


def case_name(world, stores):
    return '%s/%04d' % (world, stores)


def conditioned(world, stores):
    return (world, stores) not in ILL_CONDITIONED


def case_T(world, stores):
    """T of the world after ``stores`` stores along ``walk_stores(tabs, stores, WALK_SEED)``
    (memory/pma.py:135-139, :163-166, as tests/pma_common.py restates them)."""
    tabs, sas = pc.tables_of(WORLDS[world]())
    mem = pc.RefPMAMemory(sas, None)
    for s, a, r, ns, t in pc.walk_stores(tabs, stores, WALK_SEED):
        mem.store({'state': int(s), 'action': int(a), 'reward': float(r), 'next_state': int(ns),
                   'terminal': int(t)})
    return np.array(mem.T, dtype=np.float64)


def ring_two_absorbing():
    """A ring of six states, 0 and 3 absorbing: the eigenvalue 1 is double, the system singular."""
    T = np.zeros((6, 6))
    for s in range(6):
        if s in (0, 3):
            T[s, s] = 1.0
        else:
            T[s, (s - 1) % 6] = T[s, (s + 1) % 6] = 0.5
    return T


def tree_sum(values, dtype=np.float64):
    """The kernel's sum of S values: padded with zeros to the next power of two P, then
    v[i] += v[i + h] for h = P / 2, P / 4 .. 1."""
    S = len(values)
    P = 1
    while P < S:
        P *= 2
    v = np.zeros(P, dtype=dtype)
    v[:S] = values
    h = P // 2
    while h >= 1:
        v[:h] = v[:h] + v[h:2 * h]
        h //= 2
    return v[0]


def _solve(T, dtype):
    """(|x| / ||x||_2, status) of the bordered system in ``dtype``, operation for operation what
    k_pma_stationary does: the augmented matrix A[r][c] = ((r == c) - T[c][r]) + 1 / S with the
    right-hand side 1 / S as column S; per pivot k the largest |A[r][k]|, r >= k, the lowest row
    winning ties; the rows swapped; multipliers A[r][k] / pivot; A[r][c] - f[r] * A[k][c]; the
    back-substitution by columns, k descending; |x|; the squares summed by ``tree_sum``."""
    T = np.asarray(T, dtype=dtype)
    S = T.shape[0]
    one = dtype(1.0)
    uniform = np.full(S, one / np.sqrt(dtype(S)), dtype=dtype)
    w = one / dtype(S)
    A = np.empty((S, S + 1), dtype=dtype)
    A[:, :S] = (np.eye(S, dtype=dtype) - T.T) + w
    A[:, S] = w
    D = np.empty(S, dtype=dtype)
    with np.errstate(all='ignore'):
        for k in range(S):
            p = k + int(np.argmax(np.abs(A[k:, k])))
            pv = A[p, k]
            if pv == 0.0:
                return uniform, 1
            if p != k:
                A[[k, p]] = A[[p, k]]
            D[k] = pv
            f = A[k + 1:, k] / pv
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - f[:, None] * A[k, k + 1:][None, :]
        b = A[:, S].copy()
        x = np.empty(S, dtype=dtype)
        for k in range(S - 1, -1, -1):
            x[k] = b[k] / D[k]
            b[:k] = b[:k] - A[:k, k] * x[k]
        a = np.abs(x)
        v = a / np.sqrt(tree_sum(a * a, dtype))
    if not np.isfinite(v).all():
        return uniform, 1
    return v, 0


def stationary_ref(T):
    """``cobel_pma_stationary`` of one instance in NumPy float64: (need [S], status)."""
    return _solve(T, np.float64)


def exact(T):
    """The same system in ``np.longdouble`` (80-bit on x86): the vector, not rounded."""
    v, status = _solve(T, np.longdouble)
    assert status == 0
    return v


def eigen_gap(T):
    """The second-smallest |eig - 1| of T."""
    eig = np.linalg.eigvals(np.asarray(T, dtype=np.float64))
    return float(np.sort(np.abs(eig - 1))[1])


def residual(x, T):
    """max |x T - x| in float64."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.abs(x @ np.asarray(T, dtype=np.float64) - x).max())
