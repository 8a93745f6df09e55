"""CPU tests of the stationary-distribution need (csrc/pma_need.hip, ``PMAMemory.offline_need``):
the NumPy restatement of the kernel against the real reference's recorded vectors and an 80-bit
solution, the degenerate rule, the fixture, the exports, the plan and every refusal before a
launch, and the attribute of ``PMAMemory``.

Accuracy.  With e = max |vector - exact| the restatement must reach
``e <= max(4 * e_reference, S * 2^-53)`` on the conditioned cases: the reference (LAPACK's
``geev`` through ``scipy.linalg.eig``) is the yardstick, both are backward-stable solves of the
same problem, so their forward errors share the condition number and differ by constants of the
operation order (factor 4); S * 2^-53 is the normalisation's own sum of S squares.  Every case must
give a finite, non-negative vector of 2-norm 1 within 4 * 2^-53 whose residual max |x T - x| is at
most S * 2^-52 (evaluating the residual costs up to about S * 2^-53, the solution as much again).
The measured figures are in docs/MEASUREMENTS.md."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pma_common as pc
import pma_need_common as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_pma_stationary', 'cobel_pma_plan_need')
FAKE = 0x10000           # an aligned address nobody dereferences
IDS = [nc.case_name(w, n) for w, n in nc.CASES]


@pytest.fixture(scope='module')
def Z(golden):
    return golden('pma_need')


@pytest.fixture(scope='module')
def solved(Z):
    """The restatement of every case, computed once: name -> (vector, status)."""
    return {name: nc.stationary_ref(Z[name + '/T']) for name in IDS}


def test_fixture_holds_the_cases(Z):
    assert sorted({k.rsplit('/', 1)[0] for k in Z.files}) == sorted(IDS)
    for (world, stores), name in zip(nc.CASES, IDS):
        T = Z[name + '/T']
        S = T.shape[0]
        assert T.dtype == np.float64 and T.shape == (S, S)
        assert all(Z['%s/%s' % (name, k)].shape == (S,) for k in ('need', 'exact'))
        # row-stochastic, as memory/pma.py:139 and :163-166 keep it
        assert (T >= 0).all() and np.abs(T.sum(axis=1) - 1).max() <= 4 * nc.EPS
        if not nc.conditioned(world, stores):
            assert float(Z[name + '/gap']) < nc.GAP_CONDITIONED
    assert [Z[n + '/T'].shape[0] for n in IDS[::len(nc.STORES)]] == [12, 25, 121, 128]


def test_cases_are_what_the_common_module_builds(Z):
    """The fixture's tables are the worlds and walks of pma_need_common (two of them rebuilt)."""
    for world, stores in (('small_3x4', 60), ('demo_5x5', 400)):
        assert np.array_equal(nc.case_T(world, stores), Z[nc.case_name(world, stores) + '/T'])


@pytest.mark.parametrize('name', [n for (w, s), n in zip(nc.CASES, IDS) if nc.conditioned(w, s)])
def test_accuracy_against_the_reference(Z, solved, name):
    T, ex = Z[name + '/T'], Z[name + '/exact']
    S = T.shape[0]
    x, status = solved[name]
    assert status == 0
    e_ref = float(np.abs(Z[name + '/need'] - ex).max())
    e_x = float(np.abs(x - ex).max())
    print('%s S %d gap %.3g e_reference %.1f e_restatement %.1f (units of 2^-53) ratio %.3g'
          % (name, S, float(Z[name + '/gap']), e_ref / nc.EPS, e_x / nc.EPS,
             e_x / e_ref if e_ref else np.inf))
    assert e_x <= max(4 * e_ref, S * nc.EPS)


@pytest.mark.parametrize('name', IDS)
def test_vector_properties_and_residual(Z, solved, name):
    T = Z[name + '/T']
    S = T.shape[0]
    x, status = solved[name]
    assert status == 0 and x.dtype == np.float64 and x.shape == (S,)
    assert np.isfinite(x).all() and (x >= 0).all()
    norm = float(np.sqrt(np.sum(x.astype(np.longdouble) ** 2)))
    res = nc.residual(x, T)
    print('%s norm - 1 = %.2f, residual %.2f (units of 2^-53)'
          % (name, (norm - 1) / nc.EPS, res / nc.EPS))
    assert abs(norm - 1) <= 4 * nc.EPS
    assert res <= S * 2.0 ** -52


def test_exact_is_the_long_double_solution(Z):
    for name in IDS[:7]:
        assert np.array_equal(np.asarray(nc.exact(Z[name + '/T']), dtype=np.float64),
                              Z[name + '/exact'])


def test_degenerate_ring():
    """Two absorbing states: the eigenvalue 1 is double, the elimination meets an exactly zero
    pivot, and the answer is the uniform vector with status 1."""
    T = nc.ring_two_absorbing()
    assert np.sum(np.abs(np.linalg.eigvals(T) - 1) < 1e-12) == 2
    x, status = nc.stationary_ref(T)
    assert status == 1
    assert np.array_equal(x, np.full(6, 1.0 / np.sqrt(6.0)))
    # a table that is not finite is degenerate as well, by the second rule
    T = nc.case_T('small_3x4', 10)
    T[5, 4] = np.inf
    x, status = nc.stationary_ref(T)
    assert status == 1 and np.array_equal(x, np.full(12, 1.0 / np.sqrt(12.0)))


def test_transient_states_are_served():
    """A unichain T with transient states: a chain 0 -> 1 -> 2 into the closed class {3, 4}."""
    T = np.zeros((5, 5))
    T[0, 1] = T[1, 2] = T[2, 3] = 1.0
    T[3, 3], T[3, 4], T[4, 3], T[4, 4] = 0.25, 0.75, 0.5, 0.5
    x, status = nc.stationary_ref(T)
    pi = np.array([0, 0, 0, 0.4, 0.6])
    assert status == 0 and np.abs(x - pi / np.sqrt(np.sum(pi * pi))).max() <= 5 * nc.EPS
    assert np.array_equal(nc.stationary_ref(np.ones((1, 1)))[0], np.ones(1))


def test_fixture_regenerates(tmp_path):
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if not src or not os.path.isdir(os.path.join(src, 'cobel')):
        pytest.skip('COBEL_REFERENCE_SRC is not set: the reference is not at hand')
    env = dict(os.environ, COBEL_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'gen_pma_need.py')],
                          env=env)
    fresh = open(tmp_path / 'pma_need.npz', 'rb').read()
    assert fresh == open(os.path.join(ROOT, 'tests', 'golden', 'pma_need.npz'), 'rb').read()


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


def need_bytes(S):
    """A [S][ld] at the next odd stride past S, the multipliers / tree [P], pivots and solution
    [S] each, one flag word pair."""
    P = 1
    while P < S:
        P *= 2
    return 8 * (S * ((S + 1) | 1) + P + 2 * S) + 8


@pytest.mark.parametrize('S', [1, 2, 12, 25, 64, 65, 121, 128])
def test_plan_need(S):
    from cobel_amd import _lib
    out = (C.c_int32 * 2)()
    assert _lib.lib().cobel_pma_plan_need(S, C.byref(out)) == _lib.OK
    assert (out[0], out[1]) == (need_bytes(S), 256)
    assert out[0] <= 160 * 1024


def test_plan_need_is_sized_by_the_world():
    assert need_bytes(128) == 8 * (128 * 129 + 128 + 256) + 8 == 135176
    assert need_bytes(25) < 8 * 1024 and need_bytes(12) < 2 * 1024


def test_plan_need_refusals():
    from cobel_amd import _lib
    out = (C.c_int32 * 2)()
    for S in (0, -3, 129, 1024):
        out[0] = out[1] = 7
        assert _lib.lib().cobel_pma_plan_need(S, C.byref(out)) == _lib.E_UNSUPPORTED
        assert '128 states' in _lib.lib().cobel_last_error().decode()
        assert (out[0], out[1]) == (0, 0)
    assert _lib.lib().cobel_pma_plan_need(25, None) == _lib.E_ARG


def fake_mem(S=25, n=3, flags=0, T=FAKE):
    from cobel_amd import _lib
    m = _lib.PMAMem()
    m.T, m.n, m.n_states, m.n_actions, m.flags = T, n, S, 4, flags
    return m


def test_stationary_refuses_before_any_launch():
    """Every refusal comes before the launch: this host has no GPU, the addresses are fakes."""
    from cobel_amd import _lib
    call = _lib.lib().cobel_pma_stationary
    err = lambda: _lib.lib().cobel_last_error().decode()   # noqa: E731
    assert call(None, None, FAKE, FAKE, None) == _lib.E_ARG
    for S in (129, 0, 1024):
        m = fake_mem(S=S)
        assert call(C.byref(m), None, FAKE, FAKE, None) == _lib.E_UNSUPPORTED
        assert '128 states' in err()
    m = fake_mem(flags=_lib.PMA_WIDE)
    assert call(C.byref(m), None, FAKE, FAKE, None) == _lib.E_UNSUPPORTED
    assert 'wide' in err() and '128 states' in err()
    m = fake_mem(S=200, flags=_lib.PMA_WIDE)
    assert call(C.byref(m), None, FAKE, FAKE, None) == _lib.E_UNSUPPORTED
    for n in (0, -1):
        m = fake_mem(n=n)
        assert call(C.byref(m), None, FAKE, FAKE, None) == _lib.E_RANGE
    m = fake_mem(T=None)
    assert call(C.byref(m), None, FAKE, FAKE, None) == _lib.E_ARG
    m = fake_mem()
    assert call(C.byref(m), None, None, FAKE, None) == _lib.E_ARG
    assert call(C.byref(m), None, FAKE, None, None) == _lib.E_ARG
    assert call(C.byref(m), None, FAKE + 4, FAKE, None) == _lib.E_ARG and 'misaligned' in err()
    assert call(C.byref(m), FAKE + 2, FAKE, FAKE, None) == _lib.E_ARG and 'misaligned' in err()
    assert call(C.byref(m), None, FAKE, FAKE + 1, None) == _lib.E_ARG and 'misaligned' in err()


# -- PMAMemory ---------------------------------------------------------------------------------------
def test_offline_need_takes_two_words():
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(pc.demo_world()['sas'], EpsilonGreedy(0.1))
    assert mem.offline_need == 'host' and mem.need_status is None
    mem.offline_need = 'device'
    assert mem.offline_need == 'device'
    mem.offline_need = 'host'
    for bad in ('gpu', 'Device', None, 1, ''):
        with pytest.raises(ValueError, match="'host' or 'device'"):
            mem.offline_need = bad
        assert mem.offline_need == 'host'
    assert callable(mem.stationary)


def test_wide_memory_refuses_the_device_mode():
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(pc.demo_world()['sas'], EpsilonGreedy(0.1), wide=True)
    assert mem.offline_need == 'host'
    with pytest.raises(NotImplementedError, match='128 states'):
        mem.offline_need = 'device'
    assert mem.offline_need == 'host'
    mem.offline_need = 'host'


def test_host_mode_is_the_reference_expression(Z):
    """``'host'`` before a device is bound: the vector of ``scipy.linalg.eig``, tiled, as before."""
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(pc.demo_world()['sas'], EpsilonGreedy(0.1))
    mem.T = Z['demo_5x5/0010/T']
    need = mem.compute_need(None)
    assert need.shape == (100,) and np.array_equal(need[:25], need[75:])
    # (LAPACK's bits may differ between builds; its error here is some 14 units of 2^-53)
    assert np.abs(need[:25] - Z['demo_5x5/0010/need']).max() <= 1e-12
