"""The restatement of tests/rw_common.py (Sequence, scalar policies, Rescorla-Wagner agents, with the
device's summation order) against the traces recorded from the real reference
(tests/golden/rw_traces.npz)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rw_common as rc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rw_traces.npz')
SPARSE = [n for n, c in rc.CASES.items() if not c['dense']]


@pytest.fixture(scope='module')
def Z():
    return np.load(GOLDEN)


def test_the_fixture_holds_every_case(Z):
    assert sorted({k.split('/')[0] for k in Z.files} - {'probs'}) == sorted(rc.CASES)
    for name in rc.CASES:
        assert float(Z[name + '/margin']) > 1e-12, name


@pytest.mark.parametrize('name', SPARSE)
def test_sparse_cases_equal_the_reference_exactly(Z, name):
    """Observations of at most two non-zero components, each a power of two: every product is exact
    and any summation order, fused or not, gives BLAS's sum."""
    schedule, obs = rc.CASES[name]['design']()
    assert max(int((np.asarray(o) != 0).sum()) for o in obs.values()) <= 2
    rc.assert_same_record(rc.restate_case(name), Z, name + '/', what=name)


def test_cases_cover_what_they_are_meant_to(Z):
    assert Z['threshold_reverse/index'][0] not in (0, len(Z['threshold_reverse/value']))
    assert Z['threshold_forward/index'][0] not in (0, len(Z['threshold_forward/value']))
    cut = Z['multistep_cut/end']
    assert cut.any() and not cut.all(), 'some trials must be cut by the cap, some must end'
    steps = Z['multistep_cut/steps']
    assert steps.max() == 2 and (steps[:6] <= 1).all()
    assert len(Z['demo_rw_binary/value']) == 160 and Z['demo_rw_binary/W'][0].tolist().count(0.5) >= 3
    for name in ('proportional', 'threshold', 'sigmoid'):
        a, b = Z[name + '_reverse/action'], Z[name + '_forward/action']
        assert set(a.tolist()) == {0, 1} and set(b.tolist()) == {0, 1}, name


def test_dense_case_within_the_measured_bound(Z):
    """D = 8, dense observations: the tree sum differs from BLAS's in the last bits.  Measured by
    tests/golden/gen_rw.py: the largest |W difference| is 5.55e-17; the bound is the next power of
    two above it, 2^-53; in the values 2.22e-16 (2^-51), in the final predictions 4.16e-17 (2^-54).
    Both sides are deterministic."""
    out = rc.restate_case('dense8')
    assert rc.DENSE_MEASURED < rc.DENSE_BOUND <= 2 * rc.DENSE_MEASURED
    for k in ('action', 'end', 'steps', 'index', 'position', 'reward'):
        assert np.array_equal(out[k], Z['dense8/' + k]), k
    diff = float(np.abs(out['W'] - Z['dense8/W']).max())
    print('dense8: largest |W difference| %.17g' % diff)
    assert 0 < diff <= rc.DENSE_BOUND
    # the values handed to the policy and the final predictions, bounded the same way
    for key, measured, bound in (('value', rc.DENSE_VALUE_MEASURED, rc.DENSE_VALUE_BOUND),
                                 ('predict', rc.DENSE_PREDICT_MEASURED, rc.DENSE_PREDICT_BOUND)):
        assert measured < bound <= 2 * measured, key
        diff = float(np.abs(out[key] - Z['dense8/' + key]).max())
        print('dense8: largest |%s difference| %.17g' % (key, diff))
        assert diff <= bound, key


def test_tree_sum_is_blas_s_sum_where_the_products_are_exact():
    """Why the sparse cases can be exact: with at most two non-zero products every ORDER gives the
    same sum, and where the observation components are powers of two (as in every sparse case) each
    product is exact, so a BLAS that fuses multiply and add rounds the same value too.  (With two
    inexact products a fusing BLAS differs from any unfused sum in about a quarter of the draws:
    that is why the cases are not built from random components.)"""
    for c in (rc.CASES[n] for n in SPARSE):
        for o in c['design']()[1].values():
            nz = np.asarray(o)[np.asarray(o) != 0]
            assert len(nz) <= 2 and all(np.frexp(v)[0] == 0.5 for v in nz)
    rng = np.random.default_rng(5)
    for _ in range(5000):
        D = int(rng.integers(2, 65))
        w, x = rng.normal(size=D), np.zeros(D)
        x[rng.choice(D, 2, replace=False)] = 2.0 ** rng.integers(-3, 2, 2)
        assert rc.tree_dot(w, x) == float(w @ x.T)
