"""A fixed slice of the randomised parity sweep scripts/fuzz_sfma_sets.py: SFMA launches with
per-instance parameter sets on the device against the NumPy restatement run with each instance's
own parameters, every comparison np.array_equal.  tests/test_host_sfma_sets.py asserts, without a
GPU, what this slice contains."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))

FIRSTS, CHUNK = (0, 8, 16, 24), 8          # 32 seeds


@pytest.mark.parametrize('first', FIRSTS)
def test_random_set_cases_match_the_restatement(first):
    """Worlds of 4 .. 256 states, every launch form, launch-wide switches, 1 .. 8 sets of drawn
    values and modes over 3 .. 40 instances: latencies, replayed experiences with their TD errors,
    Q, the memory's tables and the |TD| sum of three instances, bit for bit."""
    import torch
    import fuzz_sfma_sets as fz
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    failed = []
    for seed in range(first, first + CHUNK):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]
