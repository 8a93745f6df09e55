"""CPU tests of the stationary-distribution need beyond the LDS (csrc/pma_need_wide.hip,
``PMAMemory(wide=True, need_workspace=k)``): the NumPy restatement — which the wide kernels equal
bit for bit, tests/test_gpu_pma_need_wide.py — against the real reference's recorded vectors and an
80-bit solution on worlds of 129 .. 1 024 states, the inputs of the GPU tests, the exports, the plan
and every refusal before a launch, and the constructor argument.

Accuracy, by the rule of tests/test_host_pma_need.py: with e = max |vector - exact| the restatement
must reach ``e <= max(4 * e_reference, S * 2^-53)`` wherever the second-smallest |eig - 1| of T is
at least ``GAP_CONDITIONED``; the residual max |x T - x| is at most 2 * S units of 2^-53 everywhere.
The measured figures are in docs/MEASUREMENTS.md."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pma_common as pc
import pma_need_common as nc
import pma_need_wide_common as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_pma_stationary_wide', 'cobel_pma_plan_need_wide')
FAKE = 0x10000           # an aligned address nobody dereferences
IDS = [wc.case_name(w, n) for w, n in wc.CASES]


@pytest.fixture(scope='module')
def Z(golden):
    return golden('pma_need_wide')


@pytest.fixture(scope='module')
def tables(Z):
    """name -> T: the fixture's, the two of the 1 024-state world rebuilt."""
    return {name: (wc.case_T(w, n) if w == wc.BIG else Z[name + '/T'])
            for (w, n), name in zip(wc.CASES, IDS)}


@pytest.fixture(scope='module')
def solved(tables):
    """The restatement of every case, computed once: name -> (vector, status)."""
    return {name: nc.stationary_ref(tables[name]) for name in IDS}


def test_fixture_holds_the_cases(Z, tables):
    assert len(IDS) == 14 and sorted({k.rsplit('/', 1)[0] for k in Z.files}) == sorted(IDS)
    below = []
    for (world, stores), name in zip(wc.CASES, IDS):
        T = tables[name]
        S = wc.STATES[world]
        assert T.dtype == np.float64 and T.shape == (S, S)
        assert (name + '/T' in Z.files) == (world != wc.BIG)
        assert all(Z['%s/%s' % (name, k)].shape == (S,) for k in ('need', 'exact'))
        assert (T >= 0).all() and np.abs(T.sum(axis=1) - 1).max() <= 4 * nc.EPS
        if float(Z[name + '/gap']) < nc.GAP_CONDITIONED:
            below.append((world, stores))
    assert set(below) <= set(wc.BELOW_GAP) and len(wc.BELOW_GAP) <= 1
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'pma_need_wide.npz')) < 300 * 1000


def test_cases_are_what_the_common_module_builds(Z):
    for world, stores in (('seeded_3x43', 400), ('seeded_13x17', 0)):
        assert np.array_equal(wc.case_T(world, stores), Z[wc.case_name(world, stores) + '/T'])


@pytest.mark.parametrize('name', IDS)
def test_accuracy_against_the_reference(Z, tables, solved, name):
    T, ex = tables[name], Z[name + '/exact']
    S = T.shape[0]
    x, status = solved[name]
    assert status == 0
    gap = float(Z[name + '/gap'])
    e_ref = float(np.abs(Z[name + '/need'] - ex).max())
    e_x = float(np.abs(x - ex).max())
    print('%s S %d gap %.3g e_reference %.1f e_restatement %.1f (units of 2^-53) ratio %.3g'
          % (name, S, gap, e_ref / nc.EPS, e_x / nc.EPS, e_x / e_ref if e_ref else np.inf))
    if gap >= nc.GAP_CONDITIONED:
        assert e_x <= max(4 * e_ref, S * nc.EPS)


@pytest.mark.parametrize('name', IDS)
def test_vector_properties_and_residual(tables, solved, name):
    T = tables[name]
    S = T.shape[0]
    x, status = solved[name]
    assert status == 0 and x.dtype == np.float64 and x.shape == (S,)
    assert np.isfinite(x).all() and (x >= 0).all()
    norm = float(np.sqrt(np.sum(x.astype(np.longdouble) ** 2)))
    res = nc.residual(x, T)
    print('%s norm - 1 = %.2f, residual %.2f (units of 2^-53)'
          % (name, (norm - 1) / nc.EPS, res / nc.EPS))
    assert abs(norm - 1) <= 4 * nc.EPS
    assert res <= 2 * S * nc.EPS


def test_exact_is_the_long_double_solution(Z):
    for name in IDS[:3]:
        assert np.array_equal(np.asarray(nc.exact(Z[name + '/T']), dtype=np.float64),
                              Z[name + '/exact'])


def test_the_worlds_hardly_pivot_and_the_general_matrices_do(tables):
    """What the GPU tests lean on: the fixture tables swap rows 0 .. 23 times each, ``normal`` and
    ``dyadic`` at more than 90 % of the steps with partners beyond any panel or tile edge, and
    ``dyadic`` has 3 .. 5 exactly tied pivot columns."""
    for (world, _), name in zip(wc.CASES, IDS):
        if world != wc.BIG:
            st = wc.elimination_stats(tables[name])
            assert st['zero_at'] is None and st['swaps'] <= 23 and st['ties'] == 0, (name, st)
    for S in wc.GENERAL_SIZES + (320,):
        for build in (wc.normal, wc.dyadic):
            st = wc.elimination_stats(build(S))
            assert st['zero_at'] is None and st['swaps'] > 0.9 * S and st['reach'] > 100, (S, st)
            assert (3 <= st['ties'] <= 5) if build is wc.dyadic else st['ties'] == 0, (S, st)


def test_degenerate_inputs():
    """The identity loses its pivot at step 1; a ring of S - 2 states with two absorbing states at
    the last step; a ring of 70 of 150 states in the middle of the fifth panel."""
    for S in (150, 221, 256):
        assert wc.elimination_stats(np.eye(S))['zero_at'] == 1
        ring = wc.ring_absorbing(S, S - 2)
        assert np.abs(ring.sum(axis=1) - 1).max() == 0
        assert wc.elimination_stats(ring)['zero_at'] == S - 1
        x, status = nc.stationary_ref(ring)
        assert status == 1 and np.array_equal(x, np.full(S, 1.0 / np.sqrt(float(S))))
    z = wc.elimination_stats(wc.ring_absorbing(150, 70))['zero_at']
    assert z == 71 and 0 < z % wc.PANEL < wc.PANEL - 1 and wc.PANEL < z < 150 - wc.PANEL
    for seed in (1, 2):
        for S in (150, 221, 256):
            assert nc.stationary_ref(wc.regular(S, seed))[1] == 0


def test_elimination_stats_follow_the_restatement():
    """The watched steps are the restatement's: the same degenerate verdicts."""
    for T in (nc.ring_two_absorbing(), wc.dyadic(33), wc.normal(12), np.eye(5)):
        assert (wc.elimination_stats(T)['zero_at'] is not None) == (nc.stationary_ref(T)[1] == 1)


# -- the C ABI ---------------------------------------------------------------------------------------
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


def test_abi_and_record_are_unchanged():
    from cobel_amd import _lib
    assert _lib.lib().cobel_abi_version() == 1017
    assert C.sizeof(_lib.PMAMem) == 12 * 8 + 4 * 4 + 4 * 4 + 7 * 8 + 8 == 192


def largest_lds(S):
    """The panel kernel's S rows of 17 doubles, or the back substitution's 64 x 65 block, right-hand
    side, solution and tree; the tiles take 16 512 bytes."""
    P = 1
    while P < S:
        P *= 2
    return max(8 * S * 17, 8 * (64 * 65 + 2 * S + P) + 8, 16512)


@pytest.mark.parametrize('S', [1, 2, 128, 129, 150, 240, 241, 320, 1023, 1024])
def test_plan_need_wide(S):
    from cobel_amd import _lib
    out = (C.c_int64 * 4)()
    assert _lib.lib().cobel_pma_plan_need_wide(S, C.byref(out)) == _lib.OK
    assert out[0] == wc.work_bytes(S) and out[0] % 16 == 0
    assert 8 * S * (S + 1) + 4 * (S + 1) <= out[0] < 8 * S * (S + 1) + 4 * (S + 1) + 16
    assert (out[1], out[2], out[3]) == (largest_lds(S), 256, wc.PANEL)
    assert out[1] <= 160 * 1024


def test_plan_need_wide_sizes():
    assert wc.work_bytes(1024) == 8 * 1024 * 1025 + 4 * 1025 + 12 == 8400912      # 8 MiB and a row
    assert largest_lds(1024) == 139264 and largest_lds(1) == 8 * (64 * 65 + 3) + 8


def test_plan_need_wide_refusals():
    from cobel_amd import _lib
    out = (C.c_int64 * 4)()
    for S in (0, -3, 1025, 1 << 20):
        out[0] = out[1] = out[2] = out[3] = 7
        assert _lib.lib().cobel_pma_plan_need_wide(S, C.byref(out)) == _lib.E_UNSUPPORTED
        assert '1024 states' in _lib.lib().cobel_last_error().decode()
        assert list(out) == [0, 0, 0, 0]
    assert _lib.lib().cobel_pma_plan_need_wide(150, None) == _lib.E_ARG


def fake_mem(S=150, n=3, flags=0, T=FAKE):
    from cobel_amd import _lib
    m = _lib.PMAMem()
    m.T, m.n, m.n_states, m.n_actions, m.flags = T, n, S, 4, flags
    return m


def test_stationary_wide_refuses_before_any_launch():
    """Every refusal comes before the launch: this host has no GPU, the addresses are fakes."""
    from cobel_amd import _lib
    call = _lib.lib().cobel_pma_stationary_wide
    err = lambda: _lib.lib().cobel_last_error().decode()   # noqa: E731
    big = 1 << 30
    assert call(None, None, FAKE, FAKE, FAKE, big, None) == _lib.E_ARG
    for S in (1025, 0, -1, 4096):
        for flags in (0, _lib.PMA_WIDE):
            m = fake_mem(S=S, flags=flags)
            assert call(C.byref(m), None, FAKE, FAKE, FAKE, big, None) == _lib.E_UNSUPPORTED
            assert '1024 states' in err()
    for n in (0, -1):
        m = fake_mem(n=n)
        assert call(C.byref(m), None, FAKE, FAKE, FAKE, big, None) == _lib.E_RANGE
    m = fake_mem(T=None)
    assert call(C.byref(m), None, FAKE, FAKE, FAKE, big, None) == _lib.E_ARG
    m = fake_mem()
    assert call(C.byref(m), None, None, FAKE, FAKE, big, None) == _lib.E_ARG
    assert call(C.byref(m), None, FAKE, None, FAKE, big, None) == _lib.E_ARG
    assert call(C.byref(m), None, FAKE, FAKE, None, big, None) == _lib.E_ARG and 'work' in err()
    assert call(C.byref(m), None, FAKE + 4, FAKE, FAKE, big, None) == _lib.E_ARG
    assert 'misaligned' in err()
    assert call(C.byref(m), FAKE + 2, FAKE, FAKE, FAKE, big, None) == _lib.E_ARG
    assert 'misaligned' in err()
    assert call(C.byref(m), None, FAKE, FAKE + 1, FAKE, big, None) == _lib.E_ARG
    assert 'misaligned' in err()
    assert call(C.byref(m), None, FAKE, FAKE, FAKE + 4, big, None) == _lib.E_ARG
    assert 'misaligned' in err()
    for short in (wc.work_bytes(150) - 1, 0, -8):
        assert call(C.byref(m), None, FAKE, FAKE, FAKE, short, None) == _lib.E_ARG
        assert '%d bytes' % wc.work_bytes(150) in err()


# -- PMAMemory ---------------------------------------------------------------------------------------
def memory(**kw):
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    return PMAMemory(pc.demo_world()['sas'], EpsilonGreedy(0.1), **kw)


def test_need_workspace_is_opt_in():
    assert memory().need_workspace == 0 and memory(wide=True).need_workspace == 0
    assert memory(wide=True, need_workspace=3).need_workspace == 3
    for k in (1, 5):
        with pytest.raises(ValueError, match='need_workspace'):
            memory(need_workspace=k)
        with pytest.raises(ValueError, match='need_workspace'):
            memory(wide=False, need_workspace=k)
    with pytest.raises(ValueError, match='need_workspace'):
        memory(wide=True, need_workspace=-1)


def test_wide_memory_without_a_workspace_refuses_as_before():
    mem = memory(wide=True)
    with pytest.raises(NotImplementedError, match='128 states'):
        mem.offline_need = 'device'
    assert mem.offline_need == 'host'


def test_wide_memory_with_a_workspace_accepts_the_device_mode():
    mem = memory(wide=True, need_workspace=1)
    assert mem.offline_need == 'host' and mem.need_status is None
    mem.offline_need = 'device'
    assert mem.offline_need == 'device'
    mem.offline_need = 'host'
    with pytest.raises(ValueError, match="'host' or 'device'"):
        mem.offline_need = 'gpu'
    assert mem._need_work_bytes() == wc.work_bytes(25)
