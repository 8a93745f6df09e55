"""Fixed slices of the randomised parity sweep of the tabular policy kernel (scripts/fuzz_tabpol.py,
csrc/tabular_policy.hip): QAgent and DynaQ with Softmax / ExclusiveEpsilonGreedy / RandomDiscrete on
random gridworlds (to 1 024 states), graphs of 1..8 actions and stacks of worlds, scripts of
training, budgeted, test, EpsilonGreedy and world-edit operations on one agent; after every
operation up to ten instances equal the restatement bit for bit, a test session has changed
nothing, and Dyna-Q's digest is the digest of its model.  What the slices contain is asserted on
the restatement alone by tests/test_host_fuzz_tabpol.py; the seeds are tests/fuzz_tabpol_common.py's."""
import pytest

import fuzz_tabpol_common as fa

pytestmark = pytest.mark.gpu

RAN: set = set()        # the seeds the slice tests of this process have been through


def run_seed(fz, seed):
    case = fz.draw_case(seed)
    bad = fz.run_case(case)
    RAN.add(seed)
    return case, bad


@pytest.mark.parametrize('first', fa.TABPOL_FIRSTS)
def test_random_policy_kernel_cases_match_the_restatement(first):
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import fuzz_tabpol as fz
    failed = []
    for seed in range(first, first + fa.TABPOL_CHUNK):
        case, bad = run_seed(fz, seed)
        if bad:
            failed.append((fz.describe(case), bad[:4]))
    assert not failed, failed[:3]


def test_no_case_of_the_slices_is_left_out():
    """``run_case`` lists a case it leaves out (a draw within SWEEP_MARGIN of an edge of its CDF) in
    ``REFUSED``; of the slices' seeds none may be there.  (The seeds the tests above have not been
    through in this process are run here.)"""
    import fuzz_tabpol as fz
    for seed in fa.seeds():
        if seed not in RAN:
            run_seed(fz, seed)
    assert not set(fz.REFUSED) & set(fa.seeds()), fz.REFUSED
