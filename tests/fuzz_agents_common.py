"""The fixed slices of the agent sweeps (scripts/fuzz_pma.py, fuzz_anet.py, fuzz_c2d.py,
fuzz_mfec.py) that the suite runs: tests/test_gpu_fuzz_agents.py runs them on the device,
tests/test_host_fuzz_agents.py says, on the restatements alone, what they contain.  A seed names a
case for good (every draw comes from ``np.random.default_rng(seed)``)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(os.path.dirname(HERE), 'scripts'), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# PMA memory scripts: chunks of eight seeds.  Chosen so that the slice holds every action count,
# wide cases and sizes at the top of the narrow range while only two of its cases have S x A > 512
# (the restatement's cost per replayed update).
PMA_MEMORY_FIRSTS = (0, 56, 72, 312, 336)
PMA_MEMORY_CHUNK = 8
# PMA agent runs: seeds from 10^6 on, chunks of six.
PMA_AGENT_FIRSTS = (1_000_000, 1_000_006)
PMA_AGENT_CHUNK = 6
ANET_FIRSTS = (0, 10, 20, 30)
ANET_CHUNK = 10
C2D_STEP_FIRSTS = (0, 16)
C2D_STEP_CHUNK = 16
# the eight maze with a spawn polygon almost wholly inside its holes: resets fall back
C2D_FALLBACK_SEED = 279
C2D_WHEEL_SEEDS = range(1_000_000, 1_000_006)
MFEC_SEEDS = range(0, 30)
MFEC_REFUSED_CAP = 3            # of the 30
# the second range of scripts/fuzz_mfec.py: 100 to 1 024 nodes, 5 to 8 actions, capacity up to 2 048
MFEC_WIDE_FIRSTS = (1_000_000, 1_000_004, 1_000_008)
MFEC_WIDE_CHUNK = 4
WHEEL_LEFT_OUT_CAP = 0.05       # of the instance-steps of the wheel slice


def seeds(firsts, chunk):
    return [s for f in firsts for s in range(f, f + chunk)]
