"""A fixed slice of the randomised parity sweep scripts/fuzz_pma_gain.py: PMAMemory's observables
on the device (csrc/pma_gain.hip) against the NumPy restatement of tests/pma_common.py, every
comparison np.array_equal.  tests/test_host_fuzz_pma_gain.py asserts on the restatement alone what
this slice contains."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))

FIRSTS, CHUNK = (0, 10, 20, 30), 10          # 40 seeds


@pytest.mark.parametrize('first', FIRSTS)
def test_random_gain_cases_match_the_restatement(first):
    """Successor tables of up to 40 states and 1 .. 8 actions, 1 .. 5 instances with their own
    stores, masks, both gain modes, tied and continuous Q tables, shared and per-instance sequences
    of 1 .. 40 steps: the gain map, the n-step gains, three n-step updates and the action
    probabilities, bit for bit, and no counter moved."""
    import torch
    import fuzz_pma_gain as fz
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    failed = []
    for seed in range(first, first + CHUNK):
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]
