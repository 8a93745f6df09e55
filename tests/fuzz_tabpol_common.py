"""The fixed slices of the policy-kernel sweep (scripts/fuzz_tabpol.py) that the suite runs:
tests/test_gpu_fuzz_tabpol.py runs them on the device, tests/test_host_fuzz_tabpol.py says, on the
restatement alone, what they contain.  A seed names a case for good (every draw of a case comes from
``np.random.default_rng`` seeded by it).  Chunks of forty seeds: the restatement of one chunk takes
about 5 s (docs/MEASUREMENTS.md section 35).  The last chunk holds the sweep's first world of one
state (seed 322)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(os.path.dirname(HERE), 'scripts'), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TABPOL_FIRSTS = (0, 40, 80, 120, 320)
TABPOL_CHUNK = 40
# the seeds recorded from the reference (tests/golden/gen_tabpol_sweep.py), instance 0 of each
TABPOL_RECORDED = (3, 4, 6, 11, 19, 29, 38, 39, 81, 94, 119, 125, 131, 147, 148)


def seeds(firsts=TABPOL_FIRSTS, chunk=TABPOL_CHUNK):
    return [s for f in firsts for s in range(f, f + chunk)]


def ends_mid_trial(case: dict, snaps: list) -> bool:
    """Whether a budgeted launch of the case ends inside a trial of the restated instance whose
    snapshots (one per operation) are ``snaps``."""
    done = 0
    for k, op in enumerate(case['ops']):
        if op['op'] == 'edit':
            continue
        lat = np.asarray(snaps[k]['steps'][done:done + op['trials']])
        done += op['trials']
        if op['op'] == 'train_budget':
            ends = np.cumsum(lat + 1)
            if set(range(op['budget'], int(ends[-1]), op['budget'])) - set(int(e) for e in ends):
                return True
    return False
