"""CPU tests of the device metrics (csrc/metric.hip, ``SR`` / ``DR`` with ``compute='device'``): the
NumPy restatement of tests/metric_common.py — which the kernels equal bit for bit,
tests/test_gpu_metric_*.py — against (a) the real reference's recorded matrices and (b) an 80-bit
solution; the exports, limits and the plan against the header; every refusal before a launch; the
host path unchanged; the constructor arguments.

Accuracy (b): with D80 the same elimination in np.longdouble, e_host = max |np.linalg.inv - D80|
(for DR: the host Woodbury path) and e_dev = max |restatement - D80|, the restatement must reach
``e_dev <= F * max(e_host, 2^-53 max |D80|)`` with F = 15.4, twice the worst ratio measured over
the cases below where the factor was set (7.70: DR on the world with isolated cells at gamma 0.999,
where the Woodbury correction itself loses six digits on both paths: e_host 2.8e-10, e_dev 2.2e-9).
e_dev is the same on every machine, e_host is LAPACK's and is not: on a second machine the worst
ratio was 10.99 (DR on the 10 x 10 maze, e_host 5.1e-15 there against 8.4e-15, e_dev 5.6e-14).  That
figure is the open field's D0 — 3.6 times further from the 80-bit solution by Gauss-Jordan without
pivoting than by LAPACK, 5.2e-15 against 1.5e-15 — carried through the Woodbury identity, which
multiplies either D0's error by about ten on that world: the host's Woodbury products on the
restatement's D0 give 5.2e-14 as well, the restatement's on LAPACK's D0 8.4e-15.  The tables are
in docs/MEASUREMENTS.md section 28."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import metric_common as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_metric_sr', 'cobel_metric_dr', 'cobel_metric_plan')
FAKE = 0x10000           # an aligned address nobody dereferences
GOLDEN_WORLDS = ('sfma_5x5', 'sfma_6x7')


def golden_world(Z, wname):
    nxt = Z['world/%s/next' % wname].astype(np.int32)
    W, H = int(Z['world/%s/width' % wname]), int(Z['world/%s/height' % wname])
    inv = [tuple(int(x) for x in t) for t in Z['world/%s/invalid_transitions' % wname]]
    return W, H, nxt, inv


# -- (a) the reference's matrices ------------------------------------------------------------------------
@pytest.mark.parametrize('wname', GOLDEN_WORLDS)
def test_restatement_against_the_reference(golden, wname):
    Z = golden('sfma_traces')
    W, H, nxt, inv = golden_world(Z, wname)
    assert len(mc.affected(inv)) == {'sfma_5x5': 6, 'sfma_6x7': 8}[wname]
    sr, dr = mc.sr_ref(nxt, 0.9), mc.dr_ref(W, H, nxt, inv, 0.9)
    print('%s SR %.3g DR %.3g' % (wname, np.abs(sr - Z['metric/%s/SR' % wname]).max(),
                                  np.abs(dr - Z['metric/%s/DR' % wname]).max()))
    np.testing.assert_allclose(sr, Z['metric/%s/SR' % wname], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dr, Z['metric/%s/DR' % wname], rtol=1e-12, atol=1e-14)


# -- (b) the 80-bit solution -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def solved():
    """name -> per metric (e_host, e_dev, floor), computed once."""
    from cobel_amd.memory.utils import DR, SR
    out = {}
    for name in mc.CASES:
        w, h, nxt, inv, gamma = mc.case_world(name)
        ex = mc.exact(nxt, gamma)
        out[name] = {
            'k': len(mc.affected(inv)), 'S': w * h,
            'SR': mc.errors(mc.sr_ref(nxt, gamma), SR(nxt, gamma).D, ex),
            'DR': mc.errors(mc.dr_ref(w, h, nxt, inv, gamma), DR(w, h, nxt, gamma, inv).D, ex)}
    return out


@pytest.mark.parametrize('metric', ['SR', 'DR'])
@pytest.mark.parametrize('name', list(mc.CASES))
def test_accuracy_against_80_bits(solved, name, metric):
    e_host, e_dev, floor = solved[name][metric]
    ratio = e_dev / max(e_host, floor)
    print('%s %s S %d k %d e_host %.3g e_dev %.3g floor %.3g ratio %.2f'
          % (name, metric, solved[name]['S'], solved[name]['k'], e_host, e_dev, floor, ratio))
    assert solved[name]['k'] <= mc.MAX_RANK
    assert e_dev <= mc.F * max(e_host, floor)


def test_refinement_is_the_80_bit_solution():
    """``refined`` — what the GPU tests measure against where the 80-bit elimination takes too long
    — equals ``exact`` to 2^-58 of the largest entry on the cases up to gamma 0.99."""
    from cobel_amd.memory.utils import SR
    for name in list(mc.CASES)[:4]:
        w, h, nxt, inv, gamma = mc.case_world(name)
        ex = mc.exact(nxt, gamma)
        rf = mc.refined(nxt, gamma, SR(nxt, gamma).D)
        assert float(np.abs(rf - ex).max()) <= 2.0 ** -58 * float(np.abs(ex).max()), name


def test_pivoted_inverse_swaps_and_inverts():
    rng = np.random.default_rng(5)
    for k in (1, 2, 7, 33):
        A = rng.normal(size=(k, k))
        assert np.abs(mc.pivoted_inverse(A) @ A - np.eye(k)).max() < 1e-10
    A = np.array([[0.0, 2.0], [4.0, 1.0]])          # a zero pivot without the swap
    assert np.allclose(mc.pivoted_inverse(A), np.linalg.inv(A), rtol=1e-15, atol=0)
    A = np.array([[1.0, 2.0, 0.0], [-1.0, 0.0, 1.0], [1.0, 1.0, 1.0]])   # ties: the lowest row
    assert np.abs(mc.pivoted_inverse(A) @ A - np.eye(3)).max() < 1e-15


def test_world_builders():
    nxt, inv = mc.with_walls(5, 5, [(6, 7), (7, 12)])
    assert nxt[6, 2] == 6 and nxt[7, 0] == 7 and nxt[7, 3] == 7 and nxt[12, 1] == 12
    assert list(mc.affected(inv)) == [6, 7, 12]
    for k in (0, 1, 2, 6, 8, 31, 32, 33, 128):
        nxt, inv = mc.world_of_rank(20, 20, k, seed=k)
        assert len(mc.affected(inv)) == k and nxt.shape == (400, 4)
    nxt, inv = mc.maze(12, 12, 0.05, 6, (0, 77))
    assert (nxt[0] == 0).all() and (nxt[77] == 77).all() and not (nxt[np.arange(144) != 77] == 77).any()


# -- the C ABI ---------------------------------------------------------------------------------------------
def test_exports_agree():
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'COBEL_API\s+int\s+%s\s*\(' % name, header), name
        assert name in _lib.EXPORTS
        getattr(lib, name)
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert set(NEW) <= set(re.findall(r'\bT (cobel_\w+)', out))
    assert 'metrics.py:66-268' in header
    assert lib.cobel_abi_version() == 1017


def test_limits_are_the_headers(tmp_path):
    from cobel_amd import _lib
    exe = str(tmp_path / 'limits')
    src = ('#include "cobel_hip.h"\n#include <stdio.h>\n'
           'int main(){printf("%d %d %d\\n", COBEL_METRIC_MAX_STATES, COBEL_METRIC_MAX_RANK, '
           'COBEL_METRIC_MAX_WORLDS);}')
    subprocess.run(['gcc', '-x', 'c', '-', '-I', os.path.join(ROOT, 'include'), '-o', exe],
                   input=src.encode(), check=True)
    a, b, c = [int(x) for x in subprocess.check_output([exe]).split()]
    assert (a, b, c) == (_lib.METRIC_MAX_STATES, _lib.METRIC_MAX_RANK, _lib.METRIC_MAX_WORLDS)
    assert (a, b) == (mc.MAX_STATES, mc.MAX_RANK) == (16383, 128)
    assert b % 16 == 0


def alpha_lds(k):
    """k_dr_alpha: A at a row stride of k | 1, col, row, the pivot search's 256 values, the rows of
    delta [k][9]; int32: the search's 256 rows, the pivots, delta's columns [k][9], J."""
    return 8 * (k * (k | 1) + 2 * k + 256 + 9 * k) + 4 * (256 + k + 9 * k + k)


GJ_DIAG = 8 * (32 * 33 + 2 * 32 * 32 + 32)
GJ_TILE = GJ_DIAG + 8 * (32 * 65 + 3 * 32 * 64)


@pytest.mark.parametrize('S,rank', [(1, 0), (32, 0), (33, 0), (25, 6), (272, 33), (1024, 128),
                                    (16383, 0), (16383, 128), (40, 1)])
def test_plan(S, rank):
    from cobel_amd import _lib
    rc, out = mc.plan(S, rank)
    assert rc == _lib.OK
    lds = GJ_DIAG if S <= 32 else GJ_TILE
    if rank:
        lds = max(lds, alpha_lds(rank), 8 * (32 * 65 + 32 * 64))
    world = ((36 * rank + 7) // 8 * 8 + 8 * (9 * rank + rank * rank + 2 * rank * S) + 15) // 16 * 16
    assert out == [0 if S <= 32 else 1, lds, 256, world]
    assert out[1] <= 160 * 1024
    assert _lib.metric_work_bytes(3, S, rank) == mc.work_bytes(3, S, rank)
    assert mc.work_bytes(3, S, rank) == (12 * (1 + rank) + 15) // 16 * 16 + 3 * world


def test_the_rank_limit_is_what_the_lds_holds():
    assert alpha_lds(128) == 152064 <= 160 * 1024 < alpha_lds(144)
    assert GJ_TILE == 90880


def test_plan_refusals():
    from cobel_amd import _lib
    err = lambda: _lib.lib().cobel_last_error().decode()   # noqa: E731
    for S, rank, word in ((0, 0, 'states'), (-1, 0, 'states'), (16384, 0, '16383 states'),
                          (25, -1, 'rank'), (25, 129, 'ranks 0 .. 128')):
        out = (C.c_int64 * 4)(7, 7, 7, 7)
        assert _lib.lib().cobel_metric_plan(S, rank, C.byref(out)) == _lib.E_UNSUPPORTED
        assert word in err() and list(out) == [0, 0, 0, 0]
    assert _lib.lib().cobel_metric_plan(25, 0, None) == _lib.E_ARG


def test_sr_refuses_before_any_launch():
    """Every refusal comes before the launch: this host has no GPU, the addresses are fakes."""
    from cobel_amd import _lib
    call = _lib.lib().cobel_metric_sr
    err = lambda: _lib.lib().cobel_last_error().decode()   # noqa: E731
    assert call(None, 1, 25, 0.9, FAKE, None) == _lib.E_ARG and 'next is NULL' in err()
    assert call(FAKE, 1, 25, 0.9, None, None) == _lib.E_ARG and 'D is NULL' in err()
    assert call(FAKE + 2, 1, 25, 0.9, FAKE, None) == _lib.E_ARG and 'misaligned' in err()
    assert call(FAKE, 1, 25, 0.9, FAKE + 4, None) == _lib.E_ARG and 'misaligned' in err()
    for W in (0, -2):
        assert call(FAKE, W, 25, 0.9, FAKE, None) == _lib.E_ARG and 'n_worlds' in err()
    for gamma in (1.0, -0.1, 1.5, float('nan')):
        assert call(FAKE, 1, 25, gamma, FAKE, None) == _lib.E_ARG
        assert 'gamma' in err() and '[0, 1)' in err()
    for S in (0, -5, 16384, 1 << 20):
        assert call(FAKE, 1, S, 0.9, FAKE, None) == _lib.E_UNSUPPORTED and '16383 states' in err()
    assert call(FAKE, 65536, 25, 0.9, FAKE, None) == _lib.E_UNSUPPORTED and '65535 worlds' in err()


def dr_call(**kw):
    from cobel_amd import _lib
    J = kw.pop('J', np.array([[3, 7], [4, 0]], dtype=np.int32))
    rank = kw.pop('rank', np.array([2, 1], dtype=np.int32))
    a = dict(D0=FAKE, next=FAKE, next_default=FAKE, J=J.ctypes.data if J is not None else None,
             rank=rank.ctypes.data if rank is not None else None, max_rank=2, n_worlds=2,
             n_states=25, gamma=0.9, D=2 * FAKE, work=3 * FAKE, work_bytes=1 << 30)
    a.update(kw)
    rc = _lib.lib().cobel_metric_dr(a['D0'], a['next'], a['next_default'], a['J'], a['rank'],
                                    a['max_rank'], a['n_worlds'], a['n_states'], a['gamma'], a['D'],
                                    a['work'], a['work_bytes'], None)
    return rc, _lib.lib().cobel_last_error().decode()


def test_dr_refuses_before_any_launch():
    from cobel_amd import _lib
    for name in ('D0', 'next', 'next_default', 'D', 'work'):
        rc, msg = dr_call(**{name: None})
        assert rc == _lib.E_ARG and name + ' is NULL' in msg
    rc, msg = dr_call(rank=None)
    assert rc == _lib.E_ARG and 'rank is NULL' in msg
    rc, msg = dr_call(J=None)
    assert rc == _lib.E_ARG and 'J is NULL' in msg
    for name, off in (('D0', 4), ('D', 4), ('next', 2), ('next_default', 1), ('work', 8)):
        rc, msg = dr_call(**{name: FAKE * 4 + off})
        assert rc == _lib.E_ARG and 'misaligned' in msg, name
    rc, msg = dr_call(D=FAKE)
    assert rc == _lib.E_ARG and 'must not be D0' in msg
    rc, msg = dr_call(n_worlds=0)
    assert rc == _lib.E_ARG and 'n_worlds' in msg
    for gamma in (1.0, -1e-9, float('nan')):
        rc, msg = dr_call(gamma=gamma)
        assert rc == _lib.E_ARG and '[0, 1)' in msg
    for S in (0, 16384):
        rc, msg = dr_call(n_states=S)
        assert rc == _lib.E_UNSUPPORTED and '16383 states' in msg
    rc, msg = dr_call(max_rank=-1)
    assert rc == _lib.E_ARG and 'max_rank' in msg
    rc, msg = dr_call(max_rank=129, J=np.zeros((2, 129), dtype=np.int32))
    assert rc == _lib.E_UNSUPPORTED and 'up to 128' in msg
    rc, msg = dr_call(rank=np.array([2, 129], dtype=np.int32))
    assert rc == _lib.E_UNSUPPORTED and 'world 1 has rank 129' in msg
    for bad in (3, -1):
        rc, msg = dr_call(rank=np.array([bad, 1], dtype=np.int32))
        assert rc == _lib.E_ARG and 'world 0 has rank %d' % bad in msg
    rc, msg = dr_call(J=np.array([[7, 3], [4, 0]], dtype=np.int32))
    assert rc == _lib.E_ARG and 'not sorted' in msg
    rc, msg = dr_call(J=np.array([[3, 3], [4, 0]], dtype=np.int32))
    assert rc == _lib.E_ARG and 'not sorted' in msg
    for bad in (25, -1, 1 << 20):
        rc, msg = dr_call(J=np.array([[3, 7], [bad, 0]], dtype=np.int32))
        assert rc == _lib.E_ARG and 'world 1: J[0] = %d is no state' % bad in msg
    need = mc.work_bytes(2, 25, 2)
    for short in (need - 1, 0, -16):
        rc, msg = dr_call(work_bytes=short)
        assert rc == _lib.E_ARG and '%d bytes' % need in msg
    # (the entry past a world's rank is not looked at)
    rc, msg = dr_call(J=np.array([[3, 7], [4, -9]], dtype=np.int32), n_states=0)
    assert rc == _lib.E_UNSUPPORTED


# -- the Python classes ------------------------------------------------------------------------------------
def test_host_path_is_unchanged(golden):
    """``compute='host'`` — the default — gives the arrays of the expressions it always ran."""
    from cobel_amd.memory.utils import DR, SR
    Z = golden('sfma_traces')
    for wname in GOLDEN_WORLDS:
        W, H, nxt, inv = golden_world(Z, wname)
        S = W * H
        T = mc.transition_matrix(nxt)
        want_sr = np.linalg.inv(np.eye(S) - 0.9 * T)
        T0 = mc.transition_matrix(mc.open_table(W, H))
        D0 = np.linalg.inv(np.eye(S) - 0.9 * T0)
        J = np.unique(np.array(inv)[:, 0])
        delta = (np.eye(S) - 0.9 * T)[J] - (np.eye(S) - 0.9 * T0)[J]
        cols = D0[:, J]
        alpha = np.linalg.inv(np.eye(len(J)) + np.matmul(delta, cols))
        want_dr = D0 - np.matmul(np.matmul(cols, alpha), np.matmul(delta, D0))
        for kw in ({}, {'compute': 'host'}):
            sr, dr = SR(nxt, 0.9, **kw), DR(W, H, nxt, 0.9, inv, **kw)
            assert sr.compute == dr.compute == 'host'
            assert isinstance(sr.D, np.ndarray) and np.array_equal(sr.D, want_sr)
            assert isinstance(dr.D, np.ndarray) and np.array_equal(dr.D, want_dr)
            assert np.array_equal(dr.D0, D0) and np.array_equal(dr.T_default, T0)
            dr.update_transitions()
            assert np.array_equal(dr.D, want_dr) and dr.B.shape == (S, S)
        assert np.array_equal(DR(W, H, nxt, 0.9, inv, T0).D, want_dr)
        assert np.array_equal(DR(W, H, nxt, 0.9, inv, T_default=T0, compute='host').D, want_dr)
        assert np.array_equal(dr.default_table(), mc.open_table(W, H))


def test_compute_argument():
    from cobel_amd.memory.utils import DR, SR
    nxt = mc.open_table(4, 3)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        SR(nxt, 0.9, compute='gpu')
    with pytest.raises(ValueError, match="'host' or 'device'"):
        DR(4, 3, nxt, 0.9, [], compute='cuda')


def test_device_refusals_need_no_gpu():
    """What the device form does not serve is refused on the host, with the cause, before a device
    is looked for; the host path takes all of it."""
    from cobel_amd.memory.utils import DR, SR
    nxt, inv = mc.with_walls(5, 5, [(6, 7)])
    for gamma in (1.0, -0.5, 1.2):
        with pytest.raises(ValueError, match=r'\[0, 1\)'):
            SR(nxt, gamma, compute='device')
        with pytest.raises(ValueError, match=r'\[0, 1\)'):
            DR(5, 5, nxt, gamma, inv, compute='device')
    sas = np.zeros((25, 4, 25))
    sas[np.arange(25)[:, None], np.arange(4)[None, :], nxt] = 1.0
    sas[3, 1, :] = 0.0
    sas[3, 1, 2] = sas[3, 1, 4] = 0.5
    with pytest.raises(NotImplementedError, match='distributions'):
        SR(sas, 0.9, compute='device')
    with pytest.raises(NotImplementedError, match='distributions'):
        DR(5, 5, sas, 0.9, inv, compute='device')
    assert SR(sas, 0.9).D.shape == (25, 25)
    with pytest.raises(NotImplementedError, match='T_default'):
        DR(5, 5, nxt, 0.9, inv, T_default=mc.transition_matrix(mc.open_table(5, 5)),
           compute='device')
    big = np.zeros((16384, 4), dtype=np.int32)
    with pytest.raises(NotImplementedError, match='16383'):
        SR(big, 0.9, compute='device')
    wide, wide_inv = mc.world_of_rank(20, 20, 130, seed=1)
    with pytest.raises(NotImplementedError, match='up to 128'):
        DR(20, 20, wide, 0.9, wide_inv, compute='device')
    with pytest.raises(NotImplementedError, match='up to 128'):
        DR(20, 20, [mc.open_table(20, 20), wide], 0.9, [[], wide_inv], compute='device')
    with pytest.raises(ValueError, match='one list per world'):
        DR(5, 5, [nxt, nxt], 0.9, [inv], compute='device')
    with pytest.raises(ValueError, match='width x height'):
        DR(5, 4, nxt, 0.9, inv, compute='device')
    assert DR(20, 20, wide, 0.9, wide_inv).D.shape == (400, 400)


def test_dense_one_hot_tables_reduce_to_the_compact_form():
    from cobel_amd.memory.utils import metrics
    nxt, _ = mc.with_walls(5, 5, [(6, 7), (12, 17)])
    sas = np.zeros((25, 4, 25))
    sas[np.arange(25)[:, None], np.arange(4)[None, :], nxt] = 1.0
    tabs, stacked = metrics._compact_stack(sas)
    assert not stacked and tabs.dtype == np.int32 and np.array_equal(tabs[0], nxt)
    tabs, stacked = metrics._compact_stack(nxt.astype(np.int64))
    assert not stacked and np.array_equal(tabs[0], nxt)
    for stack in ([nxt, mc.open_table(5, 5)], np.stack([nxt, mc.open_table(5, 5)]), [sas, nxt]):
        tabs, stacked = metrics._compact_stack(stack)
        assert stacked and tabs.shape == (2, 25, 4) and np.array_equal(tabs[0], nxt)
    with pytest.raises(IndexError):
        metrics._compact_stack(np.full((25, 4), 25))


def test_device_mode_without_a_gpu_fails_as_the_other_device_modules_do():
    """Without a GPU the device is what is missing (torch's own error, as for a Gridworld); with
    one, the matrix is a float64 tensor on it."""
    import torch
    from cobel_amd.memory.utils import SR
    nxt = mc.open_table(5, 5)
    if torch.cuda.is_available():
        D = SR(nxt, 0.9, compute='device').D
        assert D.is_cuda and D.dtype == torch.float64 and tuple(D.shape) == (25, 25)
    else:
        with pytest.raises((RuntimeError, AssertionError)):
            SR(nxt, 0.9, compute='device')
