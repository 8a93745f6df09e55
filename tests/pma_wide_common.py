"""Helpers of the tests of PMA's wide form (worlds of 129 ... 1 024 states): the worlds, the script of
memory calls the fixture records, and how the fixture's SR rows become the matrix a replay reads.
The restatement of tests/pma_common.py holds no 8-bit assumption and is used as it is."""
import numpy as np

import pma_common as pc

SEED = 0xC0BE1


def _world(height, width, start, goal, walls):
    from cobel_amd.misc.gridworld_tools import make_gridworld
    inv = []
    for a, b in walls:
        inv += [(a, b), (b, a)]
    w = make_gridworld(height, width, terminals=[goal], rewards=np.array([[goal, 10]]), goals=[goal],
                       invalid_transitions=inv)
    w['starting_states'] = np.array([start])
    return w


def world_132():
    """12 x 11: past 128 states (and past 127, the end of a signed byte).  Start 129 and the rewarded
    terminal state 123 lie in the last row (121 ... 131), a wall between columns 6 and 7 of the last
    two rows lies between them."""
    return _world(12, 11, 129, 123, [(10 * 11 + 6, 10 * 11 + 7), (11 * 11 + 6, 11 * 11 + 7)])


def world_272():
    """17 x 16: past 255, the first size at which an 8-bit field of a record truncates.  Start 259 and
    the rewarded terminal state 268 lie in the last row (256 ... 271), one wall segment between
    columns 7 and 8 of the last three rows lies between them."""
    return _world(17, 16, 259, 268, [(r * 16 + 7, r * 16 + 8) for r in (14, 15, 16)])


def world_1024():
    """32 x 32, four actions: the top of the range.  Start 1 000, rewarded terminal state 1 010."""
    return _world(32, 32, 1000, 1010, [(r * 32 + 12, r * 32 + 13) for r in (30, 31)])


WORLDS = {'wide_12x11': world_132, 'wide_17x16': world_272}
# name: (world, instance, stores, repeat, start state)
MEMORY_CASES = {
    'mem_wide_12x11': ('wide_12x11', 2, 40, (7, 2), 129),
    'mem_wide_17x16': ('wide_17x16', 5, 40, (8, 3), 259),
}
AGENT_WORLD, AGENT_INSTANCE, AGENT_TRIALS, AGENT_STEPS, AGENT_BATCH = 'wide_12x11', 0, 8, 3000, 8


def replay_states(ops):
    """Per replay of a script its ``current_state`` (None: the need vector is given)."""
    return [op[2] for op in ops if op[0] == 'replay']


def sr_of_row(S, state, row):
    """The SR a replay with ``current_state`` = state reads: that row, zeros elsewhere (the fixture
    keeps the rows in use, not 15 matrices of S x S doubles)."""
    sr = np.zeros((S, S))
    if state is not None:
        sr[state] = row
    return sr


def sr_bound(S, gamma):
    """|device SR - numpy.linalg.inv| as tests/test_gpu_pma.py::test_update_sr_against_inverse
    derives it: I - gamma T has norm <= 1 + gamma and its inverse <= 1 / (1 - gamma), so the
    condition is <= (1 + gamma) / (1 - gamma) and the entries are <= 1 / (1 - gamma); the error is
    of order S * 2^-53 * condition * entries, and the bound asserted is a hundred times that order,
    the margin that test leaves (1e-12 -> 1e-10, 1e-9 -> 1e-8)."""
    return 100.0 * S * 2.0 ** -53 * (1.0 + gamma) / (1.0 - gamma) / (1.0 - gamma)
