"""Trial ends of the persistent-workgroup Dyna-Q kernel (csrc/tabular_pwg.hip).  The kernel works
out where trial k + 1 starts when trial k begins and carries that start — the state and its world
record words — to the trial end, inside one ticket.  Every case runs the same inputs through that
kernel and through the wave-per-instance kernel (F_NO_PWG), which draws a start when it needs it,
and compares tables, digests, instance records (so the ENV counter), monitors and counters bit for
bit after every launch."""
import numpy as np
import pytest

import pwg_trial_ends_common as C

pytestmark = pytest.mark.gpu

# 26 x 26: the smallest square world on which the persistent kernel runs, and no power of two
SIDES = (32, 26)
N = 40


def _three_nearby(side):
    return lambda: [C.goal_nearby(side, shift) for shift in (0, 2, -3)]


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('spt', [1, 2, 3])
def test_short_trials(side, spt):
    """Trial ends back to back: the start carried for trial k + 1 is needed the step after it was
    requested (spt = 1: in the very next step, every step)."""
    from cobel_amd import _lib
    plain = C.both(_three_nearby(side), N, [64, 5, 130], spt=spt, eps=0.3)
    inst = plain['last']['inst']
    # at least a trial every `spt` steps, and every begun trial drew one start
    assert (inst[:, _lib.I_TRIAL] >= (64 + 5 + 130) // spt).all()
    assert (inst[:, _lib.I_CTR_ENV] >= inst[:, _lib.I_TRIAL]).all()


def _start_lists(side):
    """Start lists of length 1, 2 and several hundred, one per world."""
    mid = side // 2
    goal = mid * side + mid
    every = [s for s in range(side * side) if s != goal]
    return lambda: [C.goal_field(side, [goal - 4]), C.goal_field(side, [goal + 3, goal - 2 * side]),
                    C.goal_field(side, every)]


@pytest.mark.parametrize('side', SIDES)
def test_start_lists_of_every_length(side):
    from cobel_amd import _lib
    launches = [130, 7, 13, 130, 50, 9]
    plain = C.both(_start_lists(side), N, launches, spt=12, eps=0.3)
    assert len(_start_lists(side)()[2]['starting_states']) > 300
    ce = [plain['start'][:, _lib.I_CTR_ENV].astype(np.int64)] + [s['inst'][:, _lib.I_CTR_ENV].astype(np.int64)
                                          for s in plain['shots']]
    # nine trial ends and more per instance inside one launch: the ENV block (ce >> 2) changes there
    assert ((ce[1] - ce[0]) >= 9).all() and ((ce[4] - ce[3]) >= 9).all()
    assert ((ce[1] >> 2) - (ce[0] >> 2) >= 2).all()
    # launches begin at every position in a block
    assert {int(c) & 3 for at in ce[:-1] for c in at} == {0, 1, 2, 3}


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('target', [1, 2, 7])
def test_trials_target_in_the_middle_of_a_launch(side, target):
    """The target is reached inside the first launch: the start carried for the trial after it is
    dropped, and the ENV counter stays where the reference leaves it.  A second launch with a
    larger target carries on exactly: the draw not used is drawn again, none is skipped."""
    from cobel_amd import _lib
    plain = C.both(_start_lists(side), N, [(130, target), (130, target + 5)], spt=12, eps=0.3)
    first, second = plain['shots']
    ce0 = plain['start'][:, _lib.I_CTR_ENV]
    assert (first['inst'][:, _lib.I_TRIAL] == target).all()
    assert (first['inst'][:, _lib.I_STEPS_LO] <= 12 * target).all()     # (stopped well inside the launch)
    assert (first['inst'][:, _lib.I_CTR_ENV] == ce0 + target).all()           # trials begun, none ahead
    assert (second['inst'][:, _lib.I_TRIAL] == target + 5).all()
    assert (second['inst'][:, _lib.I_CTR_ENV] == ce0 + target + 5).all()


@pytest.mark.parametrize('side', SIDES)
def test_budgets_that_end_at_a_trial_end(side):
    """Trials of ten steps (obstacle mazes: few reach the goal that soon): the first budget ends
    exactly on a trial's last step, the second one step later."""
    from cobel_amd import _lib
    plain = C.both(lambda: C.mazes(side), N, [40, 41, 9, 130], spt=10)
    a, b = plain['shots'][0]['inst'], plain['shots'][1]['inst']
    on_the_end = (a[:, _lib.I_TRIAL] == 4) & (a[:, _lib.I_STEP] == 0)
    assert on_the_end.sum() >= N // 4
    # (a trial end on the budget's last step begins the next trial: its start is drawn)
    assert (a[on_the_end, _lib.I_CTR_ENV] == plain['start'][on_the_end, _lib.I_CTR_ENV] + 5).all()
    assert ((b[:, _lib.I_TRIAL] == 8) & (b[:, _lib.I_STEP] == 1)).any()


def test_sliced_launch(monkeypatch):
    """Slices are tickets of their own: each starts from the instance record.  Trials of at most
    eight steps end in every slice."""
    from cobel_amd import _lib
    # (a launch is sliced only when every CU has a workgroup: 256 x 10 wave slots)
    n, launches = 2600, [67, 67]
    worlds = lambda: C.mazes(32)   # noqa: E731
    plain = C.run(_lib.F_NO_PWG, worlds, n, launches, spt=8)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG_SLICES', '33,21,13')
    try:
        sliced = C.run(0, worlds, n, launches, spt=8)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG_SLICES', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    assert set(sliced['kinds']) == {_lib.TAB_KERNEL_PWG}
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    last = plain['last']
    assert last['q'].any() and last['batches'] > 0
    assert (last['inst'][:, _lib.I_TRIAL] >= 2 * 67 // 8).all()
    for k, (a, b) in enumerate(zip(plain['shots'], sliced['shots'])):
        C.same(a, b, 'launch %d' % k)


@pytest.mark.parametrize('side', SIDES)
def test_start_list_edited_between_launches(side):
    """What is carried does not outlive a launch: trials of the second launch start from the list
    as edited after the first."""
    from cobel_amd import _lib
    mid = side // 2
    new = [[side + 1], [2 * side + 2, 2 * side + 3], [3 * side + k for k in range(1, 9)]]

    def edit(env):
        for w, starts in zip(env.worlds, new):
            w['starting_states'] = np.array(starts)

    plain = C.both(_start_lists(side), N, [50, 60], spt=5, eps=0.3, between={1: edit})
    before, after = plain['shots'][0]['inst'], plain['shots'][1]['inst']
    old = [set(int(s) for s in w['starting_states']) for w in _start_lists(side)()]
    # an instance whose launch ended on a trial's last step stands on the start just drawn
    fresh_before = np.flatnonzero(before[:, _lib.I_STEP] == 0)
    fresh_after = np.flatnonzero(after[:, _lib.I_STEP] == 0)
    assert len(fresh_before) >= 5 and len(fresh_after) >= 5
    assert all(int(before[i, _lib.I_STATE]) in old[i % 3] for i in fresh_before)
    assert all(int(after[i, _lib.I_STATE]) in new[i % 3] for i in fresh_after)
    assert mid * side + mid not in sum(new, [])


@pytest.mark.parametrize('side', SIDES)
def test_counters_apart(side):
    """Instances whose policy and memory counters are apart take the generic step only."""
    from cobel_amd import _lib
    plain = C.both(_three_nearby(side), N, [64, 5, 130], spt=3, eps=0.3, skew=(0, 1, 2, 3))
    inst = plain['last']['inst']
    apart = (inst[:, _lib.I_CTR_POLICY] - inst[:, _lib.I_CTR_MEMORY]) & 3
    assert np.array_equal(apart, np.arange(N) & 3)
