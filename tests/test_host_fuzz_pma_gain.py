"""What the fixed slice of scripts/fuzz_pma_gain.py that tests/test_gpu_fuzz_pma_gain.py runs
contains, asserted on the NumPy restatement alone: the cases are drawn the same way on every
host, the restatement serves them all, and the slice holds tied rows, clipped and unclipped gains,
both gain modes and an ``update_q`` that breaks early."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))

import fuzz_pma_gain as fz  # noqa: E402
from test_gpu_fuzz_pma_gain import CHUNK, FIRSTS  # noqa: E402

SEEDS = [s for first in FIRSTS for s in range(first, first + CHUNK)]


def test_the_slice_is_forty_seeds():
    assert len(SEEDS) == 40 and len(set(SEEDS)) == 40


def test_cases_are_drawn_alike_every_time():
    a, b = fz.draw_case(17), fz.draw_case(17)
    assert fz.describe(a) == fz.describe(b) and np.array_equal(a['Q'], b['Q'])
    assert a['stores'] == b['stores'] and a['seqs'] == b['seqs']
    assert fz.describe(a) != fz.describe(fz.draw_case(18))


def test_what_the_slice_contains():
    cases = [fz.draw_case(s) for s in SEEDS]
    facts = [fz.run_reference(c)[1] for c in cases]
    assert sum(f['tied_rows'] for f in facts) > 0, 'no tied row'
    assert sum(f['clipped'] for f in facts) > 0 and sum(f['unclipped'] for f in facts) > 0
    assert {f['mode'] for f in facts} == {'original', 'other'}
    assert sum(f['broke'] for f in facts) > 0, 'no update_q breaks early'
    assert {c['A'] for c in cases} >= {1, 4, 8} and max(c['S'] for c in cases) == 40
    assert any(c['per_seq'] for c in cases) and any(not c['per_seq'] for c in cases)
    assert any(c['per_upd'] for c in cases) and any(c['masked'] for c in cases)
    assert any(c['Q'].ndim == 2 for c in cases) and any(c['Q'].ndim == 3 for c in cases)
    assert all(c['mask'].any(axis=1).all() for c in cases)
    assert max(len(u) for c in cases for s in c['seqs'] for u in (s if c['per_seq'] else [s])) == 40
