"""The per-step model store of the persistent-workgroup Dyna-Q kernel (csrc/tabular_pwg.hip).  A
step that re-experiences a pair with the outcome the model already holds — the digest entry in hand
equals the entry the step would write (successor | non-terminal bit, unflagged), the reward is
+0.0f and model_lr is finite — writes neither the packed record nor the digest entry.  A step that
stores takes the estimate of the pair the ticket last stored to from a register, not from the
record, which may still be on its way.  Every case runs the same seeded instances
through that kernel and through the wave-per-instance kernel (F_NO_PWG), which stores in every step,
and compares Q tables, packed records, digest, instance words and monitor sums byte for byte after
every launch."""
import numpy as np
import pytest

import pwg_model_store_common as C
from pwg_trial_ends_common import goal_field, goal_nearby, mazes

pytestmark = pytest.mark.gpu

N = 96


@pytest.mark.parametrize('side', [32, 31])
@pytest.mark.parametrize('goal', ['corner', 'middle'])
def test_first_visits_and_revisits(side, goal):
    """Fresh tables, two trials of 200 steps in one call: pairs are stored on their first visit and
    skipped on later ones (31 x 31: the instantiation for state counts that are no power of two).
    Goal in the corner: hardly an instance finds it, the steps run without planning; in the middle:
    some do, and their planning batches read the entries the steps store or skip."""
    middle = goal == 'middle'
    plain = C.both(C.one_maze(side, (side // 2) * side + side // 2 if middle else 0), N, [400],
                   spt=200, planned=middle)
    _, ns, nt, _ = C.unpack(plain['last'])
    S = side * side
    visited = (ns != np.arange(S * 4)[None, :] // 4) | (nt != 0)
    # fewer pairs than steps in every instance: some steps were revisits
    assert (visited.sum(axis=1) >= 4).all() and (visited.sum(axis=1) < 400).all()


def test_the_pair_of_the_previous_step():
    """A start cell walled in on all sides, epsilon = 1: every action bumps, the state stays, and
    the same pair repeats in consecutive steps — the digest entries in hand were requested before
    the previous step's store to that very pair.  The other start, next to the goal, fills the
    tables so that planning runs."""
    side = 32
    plain = C.both(C.cell_and_goal(side), 64, [150, 37], spt=30, eps=1.0)
    cell = 3 * side + 3
    _, ns, nt, dig = C.unpack(plain['last'])
    # the actions tried in the cell: stay, not terminal, no reward estimate
    rows = slice(cell * 4, cell * 4 + 4)
    tried = nt[:, rows] == 1
    assert tried.all(axis=1).sum() >= 32        # (half the trials start there, 30 random steps each)
    assert (ns[:, rows][tried] == cell).all() and (dig[:, rows][tried] == (cell | 0x4000)).all()


def test_flagged_pairs_keep_storing():
    """Starts one to three cells from a rewarded terminal, trials of at most three steps: the pair
    into the goal is stored while its reward estimate moves towards 1, and after that as well."""
    side = 32
    worlds = lambda: [goal_nearby(side, shift) for shift in (0, 2, -3)]   # noqa: E731
    plain = C.both(worlds, 64, [200, 131], spt=3, eps=0.3)
    rbits, _, _, dig = C.unpack(plain['last'])
    assert ((rbits != 0) == ((dig & 0x8000) != 0)).all()           # the digest mirrors the records
    est = rbits.view(np.float32)
    assert ((est > 0.5).sum(axis=1) >= 1).all()                    # every instance has found the goal
    # estimates at every stage of 1 - 0.1^k: stored again and again, not once
    assert len(np.unique(rbits[rbits != 0])) >= 4


def test_the_outcome_changes_under_a_digest_that_matched():
    """Train, then edit the live world: the reward moves to another cell, which becomes terminal,
    the old goal becomes an ordinary cell, and a third cell becomes terminal without a reward (the
    successor in the digest still matches, only the terminal bit differs).  The first steps after
    the edit must store."""
    side = 32
    mid = side // 2
    goal = mid * side + mid
    starts = [goal - 2, goal + 2 * side, goal + 3]

    def edit(env):
        for w in env.worlds:
            w['rewards'][goal] = 0.0
            w['rewards'][goal - 1] = 1.0
            w['terminals'][goal] = 0
            w['terminals'][goal - 1] = 1
            w['terminals'][goal + side] = 1

    plain = C.both(lambda: [goal_field(side, starts)], 64, [300, 200, 45], spt=12, eps=0.3,
                   between={1: edit})
    _, ns0, nt0, _ = C.unpack(plain['shots'][0])
    _, ns1, nt1, _ = C.unpack(plain['last'])
    into = lambda ns, c: ns == c   # noqa: E731
    # before the edit the unrewarded cell was entered as a non-terminal one, afterwards as a terminal
    assert (nt0[into(ns0, goal + side) & (np.arange(side * side * 4)[None, :] // 4 != goal + side)] == 1).all()
    flipped = into(ns1, goal + side) & (nt1 == 0) & (np.arange(side * side * 4)[None, :] // 4 != goal + side)
    assert flipped.any(axis=1).sum() >= 32


def test_calls_that_end_in_the_middle_of_a_trial():
    """Step budgets that are no multiple of four and end inside a trial, twice in a row: the next
    call's first step has no previous pair."""
    from cobel_amd import _lib
    plain = C.both(lambda: mazes(32), N, [131, 131, 70], spt=60)
    for shot in plain['shots'][:2]:
        assert (shot['inst'][:, _lib.I_STEP] != 0).any()


def test_sliced_launch(monkeypatch):
    """The sliced instantiations: every slice is a ticket that starts from the instance record."""
    from cobel_amd import _lib
    # (a launch is sliced only when every CU has a workgroup: 256 x 10 wave slots)
    n, launches = 2600, [67, 67]
    worlds = lambda: mazes(32)   # noqa: E731
    plain = C.run(_lib.F_NO_PWG, worlds, n, launches, spt=30)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG_SLICES', '33,21,13')
    try:
        sliced = C.run(0, worlds, n, launches, spt=30)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG_SLICES', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    assert set(sliced['kinds']) == {_lib.TAB_KERNEL_PWG}
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    assert plain['last']['batches'] > 0
    for k, (a, b) in enumerate(zip(plain['shots'], sliced['shots'])):
        C.same(a, b, 'launch %d' % k)


def test_waves_with_q_in_global_memory():
    from cobel_amd import _lib
    C.both(C.one_maze(32, 16 * 32 + 16), 64, [400], spt=200, pwg_flags=_lib.F_PWG_GLOBAL)
    C.both(C.cell_and_goal(32), 64, [150, 37], spt=30, eps=1.0, pwg_flags=_lib.F_PWG_GLOBAL)


@pytest.mark.parametrize('model_lr', [float('inf'), 1e39])
def test_model_learning_rate_that_is_not_finite(model_lr):
    """The agent accepts any learning rate of the memory.  With an infinite one (1e39: infinite as
    the float32 the kernels compute with) a step without reward makes the estimate 0 + inf * 0 =
    NaN; such a step must store, exactly as the wave-per-instance kernel does."""
    plain = C.both(C.one_maze(32, 16 * 32 + 16), N, [400], spt=200, model_lr=model_lr)
    rbits, ns, nt, dig = C.unpack(plain['last'])
    visited = (ns != np.arange(32 * 32 * 4)[None, :] // 4) | (nt != 0)
    # (inf after a first visit that was rewarded, NaN otherwise and from the second visit on)
    assert not np.isfinite(rbits.view(np.float32)[visited]).any()
    assert ((dig & 0x8000) != 0)[visited].all()
