"""Fixed slices of the randomised parity sweeps for the agents and interfaces that came after the
tabular ones: PMA / PMAMemory (scripts/fuzz_pma.py), AssociativeNetwork (fuzz_anet.py), the
continuous 2D arena (fuzz_c2d.py) and MFEC (fuzz_mfec.py), each against its float64 NumPy
restatement in tests/*_common.py.  Every comparison is np.array_equal but the wheel robot's
positions (the derived bound of tests/test_gpu_c2d.py).  tests/test_host_fuzz_agents.py asserts on
the restatements alone what these slices contain."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzz_agents_common as fa  # noqa: E402


def _sweep(fz, seeds):
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    failed = []
    for seed in seeds:
        case = fz.draw_case(seed)
        bad = fz.run_case(case)
        if bad:
            failed.append((fz.describe(case), bad))
    assert not failed, failed[:3]


@pytest.mark.parametrize('first', fa.PMA_MEMORY_FIRSTS)
def test_random_pma_memory_scripts_match_the_restatement(first):
    """scripts/fuzz_pma.py, memory cases: successor tables of 1 .. 8 actions and 1 .. 272 states
    (narrow and wide form), stores along a walk, and between them update_sr, replays of length
    1 .. 33 (from a state, from None, forced first, masked), mask and switch flips; 1 .. 65
    instances.  The device's own update_sr feeds the replays; the restatement inverts by
    pma_common.gauss_jordan.  Records, Q, generator indices, tables, SR and need, bit for bit."""
    import fuzz_pma as fz
    _sweep(fz, range(first, first + fa.PMA_MEMORY_CHUNK))


@pytest.mark.parametrize('first', fa.PMA_AGENT_FIRSTS)
def test_random_pma_agent_runs_match_the_restatement(first):
    """scripts/fuzz_pma.py, agent cases: PMA.train on seeded gridworlds of 2 x 2 to 11 x 11 (and the
    wide 12 x 11), nothing injected; latencies, the replays at trial start and end, Q, the model
    tables and the four stream indices."""
    import fuzz_pma as fz
    _sweep(fz, range(first, first + fa.PMA_AGENT_CHUNK))


@pytest.mark.parametrize('first', fa.ANET_FIRSTS)
def test_random_anet_runs_match_the_restatement(first):
    """scripts/fuzz_anet.py: every instance of every run on anet_common.EXACT."""
    import fuzz_anet as fz
    _sweep(fz, range(first, first + fa.ANET_CHUNK))


@pytest.mark.parametrize('first', fa.C2D_STEP_FIRSTS)
def test_random_arenas_step_robot_matches_the_restatement(first):
    """scripts/fuzz_c2d.py, step robot: state, reward, done, wall and counters after every step and
    reset, two lane mappings per case, sentinel frames untouched."""
    import fuzz_c2d as fz
    _sweep(fz, range(first, first + fa.C2D_STEP_CHUNK))


def test_arena_whose_spawn_area_is_a_sliver_falls_back():
    """The case at which the first run of the sweep stopped (its generator had ruled fallbacks out):
    1 024 candidates refused, the fallback point, counters + 2 052 and the device's fallback count,
    inside an ordinary walk."""
    import fuzz_c2d as fz
    _sweep(fz, [fa.C2D_FALLBACK_SEED])


def test_random_arenas_wheel_robot_within_the_derived_bound():
    """scripts/fuzz_c2d.py, wheel robot: flags, rewards and theta bit for bit, positions within
    1e-13; an instance-step is left out only where the restatement's own diagnostics show a
    decision within 1e-9 of its threshold or a hit below 0.1 rad of incidence, at most 5 % of all."""
    import fuzz_c2d as fz
    del fz.WHEEL_STATS[:]
    _sweep(fz, fa.C2D_WHEEL_SEEDS)
    total, out = sum(s[1] for s in fz.WHEEL_STATS), sum(s[2] for s in fz.WHEEL_STATS)
    worst = max(s[3] for s in fz.WHEEL_STATS)
    print('wheel robot sweep: %d of %d instance-steps left out (%.2f %%), largest position '
          'difference %.3e (bound %.0e)' % (out, total, 100.0 * out / total, worst, fz.POSITION_BOUND))
    assert len(fz.WHEEL_STATS) == len(fa.C2D_WHEEL_SEEDS)
    assert out <= fa.WHEEL_LEFT_OUT_CAP * total and worst <= fz.POSITION_BOUND


def test_random_mfec_runs_match_the_restatement():
    """scripts/fuzz_mfec.py: 30 seeds; a world the agent refuses (two nodes with allclose features)
    counts as left out, at most 3 of the 30."""
    import fuzz_mfec as fz
    del fz.REFUSED[:]
    _sweep(fz, fa.MFEC_SEEDS)
    print('MFEC sweep: %d of %d seeds refused (allclose): %s'
          % (len(fz.REFUSED), len(fa.MFEC_SEEDS), fz.REFUSED))
    assert len(fz.REFUSED) <= fa.MFEC_REFUSED_CAP


@pytest.mark.parametrize('first', fa.MFEC_WIDE_FIRSTS)
def test_random_mfec_runs_at_the_top_of_the_range_match_the_restatement(first):
    """scripts/fuzz_mfec.py, seeds from 10^6 on: random graphs of 100 to 1 024 nodes with 5 to 8
    actions, capacities of 64 to 2 048, k up to 32, lattice, one-hot or random features; none of the
    slice is refused (tests/test_host_fuzz_agents.py says what it contains)."""
    import fuzz_mfec as fz
    del fz.REFUSED[:]
    _sweep(fz, range(first, first + fa.MFEC_WIDE_CHUNK))
    assert not fz.REFUSED
