"""Helpers of the tests of ``cobel_pma_stationary_wide`` (csrc/pma_need_wide.hip): the fixture
worlds of 129 .. 1 024 states, general matrices that make the elimination swap rows at nearly every
step, degenerate inputs, and the pivoting statistics of the restatement's own steps.  The
restatement itself is ``pma_need_common.stationary_ref``, unchanged: the wide kernels owe it the
same bits as the LDS kernel does.
"""
import numpy as np

import pma_common as pc
import pma_need_common as nc

# second-smallest |eig - 1| >= 6e-4 on every case but seeded_16x20 after 3 000 stores (4.4e-5);
# seeds 1 .. 9 of the 3 x 43 world have a gap near 1e-15
WORLDS = {
    'seeded_3x43': lambda: pc.seeded_world(3, 43, 10),     # S = 129, one past the LDS kernel
    'seeded_10x15': lambda: pc.seeded_world(10, 15, 6),    # 150
    'seeded_13x17': lambda: pc.seeded_world(13, 17, 6),    # 221
    'seeded_16x20': lambda: pc.seeded_world(16, 20, 8),    # 320
    'seeded_32x32': lambda: pc.seeded_world(32, 32, 9),    # 1 024, the limit
}
STATES = {'seeded_3x43': 129, 'seeded_10x15': 150, 'seeded_13x17': 221, 'seeded_16x20': 320,
          'seeded_32x32': 1024}
STORES = (0, 400, 3000)
BIG = 'seeded_32x32'                  # its T is rebuilt by the tests, the fixture holds none
BIG_STORES = (0, 3000)
WALK_SEED = 7
MID_WORLDS = tuple(w for w in WORLDS if w != BIG)
CASES = tuple((w, n) for w in WORLDS for n in (BIG_STORES if w == BIG else STORES))
BELOW_GAP = (('seeded_16x20', 3000),)     # gap < nc.GAP_CONDITIONED: reported, not bounded
PANEL = 16                            # cobel_pma_plan_need_wide's out[3]
GENERAL_SIZES = (129, 150, 221)


def case_name(world, stores):
    return '%s/%04d' % (world, stores)


def case_T(world, stores):
    """T of the world after ``stores`` stores along ``walk_stores(tabs, stores, WALK_SEED)``."""
    tabs, sas = pc.tables_of(WORLDS[world]())
    mem = pc.RefPMAMemory(sas, None)
    for s, a, r, ns, t in pc.walk_stores(tabs, stores, WALK_SEED):
        mem.store({'state': int(s), 'action': int(a), 'reward': float(r), 'next_state': int(ns),
                   'terminal': int(t)})
    return np.array(mem.T, dtype=np.float64)


def work_bytes(S):
    """One instance's workspace as include/cobel_hip.h documents it: the augmented matrix
    [S][S + 1] of doubles, the pivot rows and one mark word, rounded up to 16 bytes."""
    return (8 * S * (S + 1) + 4 * (S + 1) + 15) // 16 * 16


# -- general matrices: the entry point does not require a stochastic T ---------------------------
def normal(S):
    return np.random.default_rng(S).standard_normal((S, S))


def dyadic(S):
    """Entries -1/4, 0, 1/4 with a unit diagonal: sums of few dyadic values, so whole pivot columns
    tie exactly."""
    T = np.random.default_rng(S).integers(-1, 2, (S, S)) * 0.25
    T[np.arange(S), np.arange(S)] = 1.0
    return T


# -- degenerate inputs --------------------------------------------------------------------------------
def ring_absorbing(S, m):
    """A ring of ``m`` states (each steps to either neighbour with probability 1/2) and ``S - m``
    absorbing states: the eigenvalue 1 has multiplicity S - m + 1."""
    T = np.zeros((S, S))
    for s in range(m):
        T[s, (s - 1) % m] += 0.5
        T[s, (s + 1) % m] += 0.5
    for s in range(m, S):
        T[s, s] = 1.0
    return T


def regular(S, seed):
    """A dense row-stochastic table: a neighbour for the degenerate instances."""
    T = np.random.default_rng(seed).uniform(0.1, 1.0, (S, S))
    return T / T.sum(axis=1, keepdims=True)


def elimination_stats(T):
    """The steps of ``pma_need_common._solve`` in float64, watched: how many steps swap rows, how far
    the farthest partner lies, how many pivot columns hold their largest magnitude more than once,
    and the first step whose pivot is exactly zero (None: none)."""
    T = np.asarray(T, dtype=np.float64)
    S = T.shape[0]
    w = 1.0 / S
    A = np.empty((S, S + 1))
    A[:, :S] = (np.eye(S) - T.T) + w
    A[:, S] = w
    out = {'swaps': 0, 'ties': 0, 'reach': 0, 'zero_at': None}
    with np.errstate(all='ignore'):
        for k in range(S):
            col = np.abs(A[k:, k])
            p = k + int(np.argmax(col))
            pv = A[p, k]
            if pv == 0.0:
                out['zero_at'] = k
                break
            out['ties'] += int(np.sum(col == col[p - k]) > 1)
            if p != k:
                out['swaps'] += 1
                out['reach'] = max(out['reach'], p - k)
                A[[k, p]] = A[[p, k]]
            f = A[k + 1:, k] / pv
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - f[:, None] * A[k, k + 1:][None, :]
    return out
