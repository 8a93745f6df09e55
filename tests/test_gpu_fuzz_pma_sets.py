"""A fixed slice of the randomised parity sweep scripts/fuzz_pma_sets.py: PMA sessions with
per-instance parameter sets on the device against the NumPy restatement run with each instance's
own ten values, every comparison np.array_equal.  tests/test_host_pma_sets.py asserts, without a
GPU, what this slice contains."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))

FIRSTS, CHUNK = (0, 8), 8          # 16 seeds


@pytest.mark.parametrize('first', FIRSTS)
def test_random_set_cases_match_the_restatement(first):
    """Gridworlds of 4 .. 42 states, 1 .. 5 sets of drawn values over 3 .. 12 instances, shared and
    separate memory policies, masked actions, one or two sessions: latencies, ``last``, every
    replay record, Q, the memory's tables, SR and the stream indices of three instances, bit for
    bit."""
    import torch
    import fuzz_pma_sets as fz
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    failed = []
    for seed in range(first, first + CHUNK):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]
