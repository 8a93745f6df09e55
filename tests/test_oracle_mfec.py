"""CPU tests: the NumPy restatement of the MFEC agent (tests/mfec_common.py) against the traces
recorded from the real reference with scikit-learn's KDTree (tests/golden/gen_mfec.py), bit for
bit.  Regenerating the fixture from the reference gives identical arrays; that is checked by hand
with the command in gen_mfec.py — these tests read only the fixture."""
import numpy as np
import pytest

import mfec_common as mc
from conftest import SEED

CASES = ['track_k3_c12', 'grid5_k10_c80', 'hex4_k2_c10', 'grid5_timeouts', 'track_c2_k3',
         'track_dict', 'track_traintest']


@pytest.fixture(scope='module')
def Z(golden):
    return golden('mfec_traces')


def test_fixture_holds_the_cases(Z):
    from conftest import cases
    assert cases(Z) == sorted(CASES)
    assert Z['hex4_k2_c10/tab_next'].shape[1] == 6
    assert str(Z['track_dict/observations']) == 'dict'
    assert int(Z['track_traintest/cfg'][5]) > 0
    for name in CASES:
        assert int(Z[name + '/buf_len'].max()) <= 80      # single-leaf trees: deterministic


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(Z, name):
    """Steps, the estimates handed to the policy, the buffers after every trial, the generator
    indices and predict_on_batch over all nodes."""
    out, _ = mc.run_restatement(mc.tables_of(Z, name), Z[name + '/F'], Z[name + '/cfg'], SEED)
    mc.assert_same_record(out, Z, name + '/', what=name)


def test_the_cases_cover_what_they_are_there_for(Z):
    # eviction and index-0 duplicates on the track
    n = 'track_k3_c12'
    lens, ids = Z[n + '/buf_len'], Z[n + '/buf_ids']
    assert (lens[-1] == 12).any()
    off = int(lens[:-1].sum())
    dup = 0
    for a, ln in enumerate(lens[-1]):
        row = ids[off:off + ln]
        dup += int((row[1:] == row[0]).sum())
        off += ln
    assert dup > 0, 'no duplicate of a buffer\'s first node'
    # some trials time out, some do not; a timed-out trial leaves the memory as it was
    n = 'grid5_timeouts'
    ended, lens = Z[n + '/ended'], Z[n + '/buf_len']
    assert ended.any() and not ended.all()
    for t in np.flatnonzero(~ended):
        if t:
            assert np.array_equal(lens[t], lens[t - 1])
    # capacity below k: no neighbour average is ever formed — an estimate is an exact hit or 0
    n = 'track_c2_k3'
    q, st = Z[n + '/q'], Z[n + '/state']
    assert int(Z[n + '/buf_len'].max()) == 2
    vals = set(np.unique(Z[n + '/buf_values']).tolist()) | {0.0}
    assert set(np.unique(q).tolist()) <= vals and len(st) == len(q)


def test_heap_order_is_not_index_order():
    """Among equidistant entries the tree's order is what the heap's pushes and the quicksort
    leave (e.g. [4, 1, 0] where a stable sort gives [0, 1, 4])."""
    seen = set()
    rng = np.random.default_rng(0)
    for _ in range(200):
        d = rng.integers(0, 3, size=8).astype(float)
        got = mc.tree_query(d, 3)
        assert sorted(d[got]) == sorted(d)[:3]
        seen.add(tuple(got) == tuple(np.argsort(d, kind='stable')[:3]))
    assert seen == {True, False}


def test_pair_tables_are_the_sequential_sum():
    rng = np.random.default_rng(1)
    F = rng.random((7, 16))
    F[3] = F[2] * (1 + 5e-5)        # allclose one way round only near the edge: not symmetric in general
    R, same = mc.pair_tables(F)
    for q in range(7):
        for j in range(7):
            d = 0.0
            for x in range(16):
                t = F[q, x] - F[j, x]
                d += t * t
            assert R[q, j] == d
            assert same[q, j] == np.allclose(F[j], F[q], rtol=1e-4, atol=1e-6)
    assert same[2, 3] and same[3, 2] and not same[0, 1]
