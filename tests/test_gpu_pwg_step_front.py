"""The front half of a step of the persistent-workgroup Dyna-Q kernel (csrc/tabular_pwg.hip): the
successor and the digest entry of the action taken are read out of per-lane registers (lane l
holds successor l % 4 and the aligned digest word that holds entry l % 4), the planning patches for
the pair a step stored to run only in steps that store, and a step ends through one scalar word
(bit 0: the trial is over, bit 1: the step stored).  Every case runs the same seeded instances
through that kernel and through the wave-per-instance kernel (F_NO_PWG) and compares Q tables,
packed records, digest, instance words and monitor sums byte for byte after every launch."""
import numpy as np
import pytest

import pwg_model_store_common as C
import pwg_trial_ends_common as T
from conftest import SEED

pytestmark = pytest.mark.gpu

N = 96
SIDES = [26, 31, 32]   # 26 x 26: the smallest world the kernel serves here; 31: no power of two


def corners_and_goal(side):
    """An open field, goal in the middle.  Trials start in the four corners (two of the four moves
    bump there, every direction in one corner or another; the last one is state S - 1, whose digest
    entries are the last of the instance's), in an interior cell (four different successors) and
    next to the goal (so that the tables fill and planning runs)."""
    S = side * side
    mid = (side // 2) * side + side // 2
    starts = [0, side - 1, S - side, S - 1, side + 1, mid - 2]
    return lambda: [T.goal_field(side, starts)]


@pytest.mark.parametrize('side', SIDES)
def test_every_action_and_every_half_of_the_record_words(side):
    """epsilon = 1: all four actions are taken everywhere, so every lane of a quad supplies the
    successor and both halves of both digest words supply the entry."""
    S = side * side
    plain = C.both(corners_and_goal(side), N, [150, 50], spt=25, eps=1.0)
    _, ns, nt, dig = C.unpack(plain['last'])
    own = np.broadcast_to(np.arange(S * 4)[None, :] // 4, ns.shape)
    tried = nt == 1                               # (an open field: only the goal is terminal)
    bumps = np.zeros(4, dtype=bool)
    for cell in (0, side - 1, S - side, S - 1):
        rows = slice(cell * 4, cell * 4 + 4)
        every = tried[:, rows].all(axis=1)        # instances that took all four actions in the corner
        assert every.any(), cell
        stay = (ns[:, rows] == cell)[every]
        assert (stay.sum(axis=1) == 2).all(), cell   # two of the four moves bump
        bumps |= stay.any(axis=0)
        assert (dig[:, rows][tried[:, rows]] & 0x4000).all()
    assert bumps.all()                            # every direction bumps somewhere
    inner = slice((side + 1) * 4, (side + 1) * 4 + 4)
    every = tried[:, inner].all(axis=1)
    assert every.any() and (np.sort(ns[:, inner][every], axis=1) ==
                            np.sort([1, side, side + 2, 2 * side + 1])).all()
    assert (ns[tried] != own[tried]).any() and plain['last']['batches'] > 0


def field_near_goal(side):
    """An open field; trials start two to four cells from the goal in its middle."""
    mid = (side // 2) * side + side // 2
    return lambda: [T.goal_field(side, [mid - 2, mid + 2 * side, mid - 3 * side - 1])]


def oracle_events(world, instances, trials, spt, batch, eps, model_lr=0.9):
    """The NumPy oracle on some instances, whole trials.  Per kind of step — one that stores its
    model record, one that skips the store (the pair was visited, no reward, estimate +0.0) — the
    planning lanes that replay the step's own pair in the batch of that step, and in the batch the
    next step runs (drawn, and its digest entries requested, in that step).  Counted in steps whose
    planning runs, that is from the instance's first reward on."""
    from oracle import philox, ref_loop
    tabs = world.compact()
    S = int(world['states'])
    out = {'cur_store': 0, 'cur_skip': 0, 'next_store': 0, 'next_skip': 0, 'rewarded_store': 0}
    for i in instances:
        env = ref_loop.RefGridworld(tabs, philox.TapeRNG(SEED, i, philox.STREAM_ENV))
        pol = ref_loop.RefEpsilonGreedy(eps, philox.TapeRNG(SEED, i, philox.STREAM_POLICY))
        ref = ref_loop.RefDynaQ(S, 4, pol, philox.TapeRNG(SEED, i, philox.STREAM_MEMORY),
                                dtype=np.float32)
        ref.M.learning_rate = model_lr
        tr = ref_loop.new_trace()
        ref.train(env, trials, spt, batch, trace=tr)
        seen, est, planning = set(), {}, False
        for t, (s, a, r, _, _) in enumerate(tr['sarsn']):
            sa = int(s) * 4 + int(a)
            skip = sa in seen and r == 0.0 and est.get(sa, 0.0) == 0.0
            seen.add(sa)
            est[sa] = np.float32(est.get(sa, np.float32(0.0)) +
                                 np.float32(model_lr) * (np.float32(r) - est.get(sa, np.float32(0.0))))
            planning = planning or r != 0.0
            if not planning:
                continue
            kind = 'skip' if skip else 'store'
            out['cur_' + kind] += int((tr['idx'][t] == sa).sum())
            if t + 1 < len(tr['idx']):
                out['next_' + kind] += int((tr['idx'][t + 1] == sa).sum())
            out['rewarded_store'] += int(r != 0.0)
    return out


@pytest.mark.parametrize('side', SIDES)
def test_planning_lanes_that_replay_the_pair_of_the_step(side):
    """Fresh tables, trials that start near the goal, epsilon = 0.5: planning runs from the first
    trials on, many steps store (first visits, the rewarded pairs into the goal), many skip, and
    with 4 S pairs and 50 planning lanes some lanes replay the very pair the step stored to or
    skipped — in the step's own batch and in the one drawn for the next step.  That all of it
    occurred is read off the oracle's trace of twelve instances, not assumed: their first six
    trials, at most 240 steps, which the launch of 300 covers."""
    from cobel_amd import _lib
    make = field_near_goal(side)
    plain = C.both(make, N, [300], spt=40, eps=0.5)
    assert (plain['last']['inst'][:12, _lib.I_TRIAL] >= 6).all()
    ev = oracle_events(make()[0], range(12), 6, 40, 50, 0.5)
    for key in ('cur_store', 'cur_skip', 'next_store', 'next_skip', 'rewarded_store'):
        assert ev[key] >= 1, (key, ev)


@pytest.mark.parametrize('model_lr', [float('inf'), 0.25])
def test_rewarded_pairs_and_a_model_learning_rate_that_is_not_finite(model_lr):
    """Starts one to three cells from the goal, short trials: the pair into the goal is flagged
    (its estimate comes from the register of the last store or from the record, in the planning
    lanes' rare block); with an infinite learning rate every step stores, estimates of inf and NaN
    reach most planning lanes, and the Q tables must hold the same NaNs, sign included (the float64
    planning update adds two NaNs of different sign there: its operand order is fixed in the
    kernel)."""
    worlds = lambda: [T.goal_nearby(26, shift) for shift in (0, 2, -3)]   # noqa: E731
    plain = C.both(worlds, N, [160, 75], spt=3, eps=0.3, model_lr=model_lr)
    rbits, _, _, dig = C.unpack(plain['last'])
    assert ((rbits != 0) == ((dig & 0x8000) != 0)).all()
    assert ((dig & 0x8000) != 0).any(axis=1).all()


def test_the_pair_of_the_previous_step():
    """A start cell walled in on all sides, epsilon = 1: a step that skips directly behind a step
    that stored to the same pair (the entry in hand is one store old)."""
    side = 26
    plain = C.both(C.cell_and_goal(side), 64, [150, 37], spt=30, eps=1.0)
    cell = 3 * side + 3
    _, ns, nt, dig = C.unpack(plain['last'])
    rows = slice(cell * 4, cell * 4 + 4)
    tried = nt[:, rows] == 1
    assert tried.all(axis=1).sum() >= 16
    assert (ns[:, rows][tried] == cell).all() and (dig[:, rows][tried] == (cell | 0x4000)).all()


@pytest.mark.parametrize('side,spt,target', [(26, 1, 140), (32, 2, 74), (31, 3, 52), (26, 5, 31),
                                             (32, 30, 5)])
def test_trial_ends_in_every_phase_behind_storing_and_skipped_steps(side, spt, target):
    """Trials of 1, 2, 3, 5 and 30 steps end in every position of a group of four; on fresh tables
    the step before the end stores, later it skips.  Budgets that end inside a group, and a trial
    target (a count of trials since the tables were fresh) reached inside the second launch."""
    worlds = lambda: T.mazes(side)   # noqa: E731
    launches = [131, (70, target), 54]
    plain = T.both(worlds, N, launches, spt=spt) if spt >= 5 else \
        T.run(0, worlds, N, launches, spt=spt)
    if spt < 5:   # (hardly an instance finds a goal in so short a trial: no demand on planning)
        from cobel_amd import _lib
        ref = T.run(_lib.F_NO_PWG, worlds, N, launches, spt=spt)
        assert set(plain['kinds']) == {_lib.TAB_KERNEL_PWG}
        assert set(ref['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
        for k, (a, b) in enumerate(zip(ref['shots'], plain['shots'])):
            T.same(a, b, 'launch %d' % k)
        plain = ref
    from cobel_amd import _lib
    trials = plain['shots'][1]['inst'][:, _lib.I_TRIAL]
    assert (trials == target).any()       # the target was reached inside the launch
    assert plain['last']['lat_cnt'].sum() > 0


def test_short_trials_with_planning():
    """Goal nearby, trials of at most 2 and 3 steps with planning running: both bits of the
    step-end word meet (a storing step that ends the trial) and each occurs alone."""
    for spt in (2, 3):
        worlds = lambda: [T.goal_nearby(26, shift) for shift in (0, 2, -3)]   # noqa: E731
        T.both(worlds, N, [131, (70, 40), 54], spt=spt, eps=0.3)


def test_counters_apart():
    """Instances whose policy counter is ahead of the memory counter take the generic step only."""
    T.both(lambda: T.mazes(26), N, [131, 54], spt=20, skew=[0, 1, 2, 3, 5])


def test_sliced_launch(monkeypatch):
    from cobel_amd import _lib
    n, launches = 2600, [67, 67]
    worlds = lambda: T.mazes(26)   # noqa: E731
    plain = C.run(_lib.F_NO_PWG, worlds, n, launches, spt=20)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG_SLICES', '33,21,13')
    try:
        sliced = C.run(0, worlds, n, launches, spt=20)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG_SLICES', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    assert set(sliced['kinds']) == {_lib.TAB_KERNEL_PWG}
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    assert plain['last']['batches'] > 0
    for k, (a, b) in enumerate(zip(plain['shots'], sliced['shots'])):
        C.same(a, b, 'launch %d' % k)


def test_a_forced_mix_with_global_memory_waves(monkeypatch):
    """Ten LDS waves and three with Q in global memory in every workgroup, and all sixteen in
    global memory."""
    from cobel_amd import _lib
    make = C.one_maze(26, 13 * 26 + 13)
    plain = C.run(_lib.F_NO_PWG, make, N, [300], spt=150)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG', '3,2')
    try:
        mixed = C.run(0, make, N, [300], spt=150)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    glob = C.run(_lib.F_PWG_GLOBAL, make, N, [300], spt=150)
    assert set(mixed['kinds']) == {_lib.TAB_KERNEL_PWG} and plain['last']['batches'] > 0
    C.same(plain['last'], mixed['last'], 'mixed')
    C.same(plain['last'], glob['last'], 'global')
    C.both(C.cell_and_goal(26), 64, [150, 37], spt=30, eps=1.0, pwg_flags=_lib.F_PWG_GLOBAL)
