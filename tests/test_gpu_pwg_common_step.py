"""The common step of the persistent-workgroup Dyna-Q kernel (csrc/tabular_pwg.hip): the online TD
value is formed outside the one-lane store, a flagged digest entry is found with one compare for the
whole wave, the Philox block of a group's last step takes its counter, lane word and stream from
lane constants, and a step's rare block hands its result on as one scalar.  Every case runs the
same seeded instances through that kernel and through the wave-per-instance kernel (F_NO_PWG) and
compares Q tables, packed records, digest, instance words and monitor sums byte for byte after
every launch."""
import numpy as np
import pytest

import pwg_model_store_common as C
import pwg_trial_ends_common as T
from conftest import SEED

pytestmark = pytest.mark.gpu

N = 96
SIDES = [26, 31, 32]   # 26 x 26: the smallest world the kernel serves here; 31: no power of two


def near_goal(side):
    return lambda: [T.goal_nearby(side, shift) for shift in (0, 2, -3)]


# ---- batch sizes ----------------------------------------------------------------------------------
@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('batch', [1, 2, 50, 61, 62])
def test_batch_sizes_next_to_the_policy_lanes(side, batch):
    """One and two planning lanes, the usual fifty, and the last lanes in front of the policy's (62
    and 63 hold its blocks): the lanes behind the batch draw and gather like the others and must
    leave nothing behind.  Budgets that are no multiples of four, 34 and 21 Philox blocks long,
    trials of at most seven steps: trial ends fall on either side of the group's last step, where
    the next blocks are evaluated."""
    C.both(near_goal(side), N, [135, 83], batch=batch, spt=7, eps=0.3)


# ---- tag rounds -----------------------------------------------------------------------------------
class _Probe:
    """RefDynaQ whose replay() also sorts every planning batch by what its first round does in the
    kernel: the lanes whose update changes their cell (writers), and the first lane that reads a
    cell an earlier writer changes (held back) — from the oracle's own table and model alone."""

    @staticmethod
    def make(S, pol, mem_rng, alpha):
        from oracle import ref_loop

        class Probe(ref_loop.RefDynaQ):
            kinds = {'no_writer': 0, 'all_commit': 0, 'held_lane_1': 0, 'held_last_lane': 0,
                     'held_elsewhere': 0, 'flagged_lanes': 0}
            planning = False

            def replay(self, batch, trace=None):
                exps, flat = self.M.sample(batch)
                if self.planning:
                    Q0 = self.Q
                    writes = {}            # cell -> earliest lane that changes it
                    held = None
                    with np.errstate(all='ignore'):
                        for j, (s, a, r, ns, nt) in enumerate(exps):
                            cell = int(s) * 4 + int(a)
                            reads = [int(ns) * 4 + k for k in range(4)] + [cell]
                            if held is None and any(c in writes for c in reads):
                                held = j
                            q = Q0[s][a]
                            td = r
                            td = td + self.gamma * nt * np.amax(Q0[ns])
                            td = td - q
                            qn = np.float32(np.float64(q) + self.learning_rate * td)
                            if qn.tobytes() != np.float32(q).tobytes():
                                writes.setdefault(cell, j)
                            self.kinds['flagged_lanes'] += int(np.float32(r).tobytes() != b'\0\0\0\0')
                    if not writes:
                        self.kinds['no_writer'] += 1
                    elif held is None:
                        self.kinds['all_commit'] += 1
                    elif held == 1:
                        self.kinds['held_lane_1'] += 1
                    elif held == batch - 1:
                        self.kinds['held_last_lane'] += 1
                    else:
                        self.kinds['held_elsewhere'] += 1
                for s, a, r, ns, nt in exps:
                    self._td(s, a, r, ns, nt)
                if trace is not None:
                    trace['idx'].append(np.asarray(flat))

        Probe.kinds = dict(Probe.kinds)
        return Probe(S, 4, pol, mem_rng, learning_rate=alpha, dtype=np.float32)


def batch_kinds(world, instances, trials, spt, batch, eps, alpha=0.99):
    """The oracle on some instances, whole trials: its planning batches by kind (from the
    instance's first reward on, where planning runs in the kernels)."""
    from oracle import philox, ref_loop
    tabs = world.compact()
    S = int(world['states'])
    total = None
    for i in instances:
        env = ref_loop.RefGridworld(tabs, philox.TapeRNG(SEED, i, philox.STREAM_ENV))
        pol = ref_loop.RefEpsilonGreedy(eps, philox.TapeRNG(SEED, i, philox.STREAM_POLICY))
        ref = _Probe.make(S, pol, philox.TapeRNG(SEED, i, philox.STREAM_MEMORY), alpha)
        store = ref.M.store

        def watch(s, a, r, ns, nt, ref=ref, store=store):
            store(s, a, r, ns, nt)
            ref.planning = ref.planning or np.float32(r).tobytes() != b'\0\0\0\0'
        ref.M.store = watch
        ref.train(env, trials, spt, batch)
        total = ref.kinds if total is None else {k: total[k] + v for k, v in ref.kinds.items()}
    return total


TAG_INSTANCES = (2, 10, 33, 37)
TAG_TRIALS, TAG_SPT = 10, 30


def test_tag_rounds_of_young_agents():
    """alpha .99, epsilon 1, 62 planning lanes on 26 x 26: fresh values change wherever planning
    looks, so batches have many writers.  The oracle, run for four of the instances, must show all
    four kinds of batch: none that writes, writers that all commit in the first round (the kernel's
    short way out), a batch held back at lane 1 and one held back at the last planning lane.  Ten
    trials of at most thirty steps: the launch of 300 steps covers them."""
    from cobel_amd import _lib
    make = lambda: [T.goal_nearby(26)]   # noqa: E731
    plain = C.both(make, N, [300, 61], batch=62, spt=TAG_SPT, eps=1.0)
    assert (plain['shots'][0]['inst'][list(TAG_INSTANCES), _lib.I_TRIAL] >= TAG_TRIALS).all()
    kinds = batch_kinds(make()[0], TAG_INSTANCES, TAG_TRIALS, TAG_SPT, 62, 1.0)
    for key in ('no_writer', 'all_commit', 'held_lane_1', 'held_last_lane'):
        assert kinds[key] >= 1, (key, kinds)


# ---- step end -------------------------------------------------------------------------------------
@pytest.mark.parametrize('side,spt,target', [(26, 1, 142), (31, 2, 110), (32, 5, 45)])
def test_step_ends_with_planning_running(side, spt, target):
    """Trials of at most 1, 2 and 5 steps that start next to the goal: trials end in every position
    of a group of four, steps store and end the trial at once (the first visit of a pair into the
    goal, and every rewarded step), and the trial target is reached inside the second launch, for
    trials of one step at its tenth step — inside a group."""
    from cobel_amd import _lib
    plain = T.both(near_goal(side), N, [131, (70, target), 54], spt=spt, eps=0.3)
    trials = plain['shots'][1]['inst'][:, _lib.I_TRIAL]
    steps = plain['shots'][1]['steps'] - plain['shots'][0]['steps']
    assert (trials == target).any() and steps < 70 * N   # some instance stopped short of its budget


# ---- rare blocks ----------------------------------------------------------------------------------
def test_rewarded_pairs_are_replayed():
    """The pairs into the goal carry an estimate: a planning lane that draws one takes it from the
    packed record or from the register of the last store (the flagged-entry block).  That such
    lanes occurred is read off the oracle."""
    make = lambda: [T.goal_nearby(26)]   # noqa: E731
    plain = C.both(make, N, [200], spt=12, eps=0.5)
    rbits, _, _, dig = C.unpack(plain['last'])
    assert ((rbits != 0) == ((dig & 0x8000) != 0)).all() and (rbits != 0).any()
    kinds = batch_kinds(make()[0], (0, 1, 2, 3), 8, 12, 50, 0.5)
    assert kinds['flagged_lanes'] >= 1, kinds


def minus_zero_field(side):
    """One terminal next to the start cells, and it pays -0.0f: a reward with bits and no value."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    mid = (side // 2) * side + side // 2
    return lambda: [make_gridworld(side, side, terminals=[mid], rewards=np.array([[mid, -0.0]]),
                                   goals=[mid], starting_states=[mid + 2, mid + 2 + side, mid - 2 - side])]


def test_a_reward_of_minus_zero():
    """The only reward of the world is -0.0f.  It has bits, so the step that meets it is a rewarded
    step (it stores, and from then on the instance's planning batches run and are counted — the
    count is compared with the reference kernel's and must not be zero), and it has no value, so
    every table stays at zero."""
    make = minus_zero_field(26)
    assert np.signbit(make()[0]['rewards']).sum() == 1
    plain = C.both(make, N, [150, 50], spt=9, eps=0.5, planned=True)
    _, ns, nt, _ = C.unpack(plain['last'])
    mid = 13 * 26 + 13
    assert ((ns == mid) & (nt == 0)).any(axis=1).sum() >= N // 2   # most instances entered the terminal
    assert not plain['last']['q'].view(np.uint32).any() or (plain['last']['q'] == 0).all()


@pytest.mark.parametrize('model_lr', [float('inf'), float('nan')])
def test_a_model_learning_rate_that_is_not_finite(model_lr):
    """Every step stores; estimates of inf and NaN reach the planning lanes, and the float64
    planning sum must return the same NaN, sign included."""
    plain = C.both(near_goal(26), N, [150, 51], spt=5, eps=0.3, model_lr=model_lr)
    assert np.isnan(plain['last']['q']).any()


@pytest.mark.parametrize('goal', [0, 13 * 26 + 13])
def test_instances_that_are_all_zero_for_their_first_steps(goal):
    """Fresh tables: nothing is planned until the instance meets its first reward.  With the goal
    in the corner few instances meet it in these launches, with the goal in the middle many do, at
    every point of a launch; the others stay all zero throughout."""
    plain = C.both(C.one_maze(26, goal), N, [150, 150], spt=150)
    found = plain['last']['q'].reshape(N, -1).any(axis=1)
    assert found.any() and not found.all()


# ---- the other instantiations ------------------------------------------------------------------------
def test_sliced_launch_with_62_planning_lanes(monkeypatch):
    from cobel_amd import _lib
    n, launches = 2600, [67, 67]
    worlds = lambda: T.mazes(31)   # noqa: E731
    plain = C.run(_lib.F_NO_PWG, worlds, n, launches, spt=20, batch=62)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG_SLICES', '33,21,13')
    try:
        sliced = C.run(0, worlds, n, launches, spt=20, batch=62)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG_SLICES', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    assert set(sliced['kinds']) == {_lib.TAB_KERNEL_PWG}
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    assert plain['last']['batches'] > 0
    for k, (a, b) in enumerate(zip(plain['shots'], sliced['shots'])):
        C.same(a, b, 'launch %d' % k)


@pytest.mark.parametrize('side,batch', [(26, 62), (31, 2), (32, 50)])
def test_generic_step_with_counters_apart(side, batch):
    """Instances whose policy counter is ahead of the memory counter take the generic step only."""
    T.both(near_goal(side), N, [131, 54], spt=9, eps=0.3, batch=batch, skew=[0, 1, 2, 3, 5])


def test_a_forced_mix_with_global_memory_waves(monkeypatch):
    """Three LDS waves and two with Q in global memory in every workgroup."""
    from cobel_amd import _lib
    make = near_goal(26)
    plain = C.run(_lib.F_NO_PWG, make, N, [203, 50], spt=9, eps=0.3, batch=61)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG', '3,2')
    try:
        mixed = C.run(0, make, N, [203, 50], spt=9, eps=0.3, batch=61)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    assert set(mixed['kinds']) == {_lib.TAB_KERNEL_PWG} and plain['last']['batches'] > 0
    for k, (a, b) in enumerate(zip(plain['shots'], mixed['shots'])):
        C.same(a, b, 'launch %d' % k)
