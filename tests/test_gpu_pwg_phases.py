"""The step loop of the persistent-workgroup Dyna-Q kernel (csrc/tabular_pwg.hip) takes its steps
in groups of four with the Philox phase known at compile time, and single generic steps wherever a
group does not fit: heads and tails of a budget, the steps after a trial's end, instances whose
policy and memory counters are apart.  Every case runs the same inputs through that kernel and
through the wave-per-instance kernel (F_NO_PWG), which knows no groups, and compares tables,
digests, instance records, monitors and counters bit for bit."""
import numpy as np
import pytest
import torch

from conftest import SEED

pytestmark = pytest.mark.gpu

KEYS = ('q', 'model', 'index', 'inst', 'lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt', 'lat_trace')
# 26 x 26: the smallest square world whose Q tables leave a CU fewer than sixteen workgroups of the
# wave-per-instance kernel (676 x 16 B in blocks of 1 280 B: fourteen), so the persistent kernel
# runs — and not a power of two, the other instantiation than 32 x 32
SIDES = (32, 26)


def _snapshot(agent):
    mon = agent.monitors
    out = {'q': agent._q, 'model': agent.M.table, 'index': agent.M.index, 'inst': agent.inst,
           'lat_sum': mon.lat_sum, 'lat_cnt': mon.lat_cnt, 'reward_sum': mon.reward_sum,
           'resp_cnt': mon.resp_cnt, 'lat_trace': mon.lat_trace}
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out['batches'] = int(agent.batches_done.item())
    out['steps'] = agent.env_steps()
    return out


def _run(extra_flags, worlds, n, budgets, batch=50, spt=60, alpha=0.99, eps=0.1,
         trials_target=0x7fffffff, skew=None):
    """One agent, one launch per entry of `budgets`; a snapshot after every launch.  `skew`: added
    to the policy counter of instance i before the first launch (skew[i % len(skew)])."""
    from cobel_amd import _lib
    from cobel_amd.agent import DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(worlds, n_envs=n, seed=SEED, device=torch.device('cuda', 0))
    agent = DynaQ(env.observation_space, env.action_space, EpsilonGreedy(eps), learning_rate=alpha)
    agent.extra_flags = extra_flags
    agent.track_instances = True
    agent.track_responses = True
    agent._bind(env)
    agent._env_in(env)
    flags = _lib.F_LEARN | agent._policy_in(agent.policy, env, False)
    agent.monitors.reserve(2048, n, True)
    if skew is not None:
        add = torch.as_tensor([skew[i % len(skew)] for i in range(n)], dtype=torch.int32,
                              device=agent.inst.device)
        agent.inst[:, _lib.I_CTR_POLICY] += add
    kinds, shots = [], []
    for budget in budgets:
        kinds.append(agent.describe_launch(env, agent.policy, flags, trials_target, spt, budget,
                                           batch)['kernel'])
        agent._launch(env, agent.policy, flags, trials_target, spt, budget, batch)
        torch.cuda.synchronize()
        shots.append(_snapshot(agent))
    return {'kinds': kinds, 'shots': shots, 'last': shots[-1]}


def _same(a, b, where=''):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (key, where)
    assert a['batches'] == b['batches'] and a['steps'] == b['steps'], where


def _both(worlds, n, budgets, **args):
    """The reference kernel and the persistent one on the same inputs, equal after every launch."""
    from cobel_amd import _lib
    plain = _run(_lib.F_NO_PWG, worlds, n, budgets, **args)
    pwg = _run(0, worlds, n, budgets, **args)
    # (a launch of ONE step reports the step's experience and is the general wavefront kernel's on
    #  either side: it only moves the counters on by one between the launches compared here)
    for budget, kp, kw in zip(budgets, plain['kinds'], pwg['kinds']):
        assert kp == (_lib.TAB_KERNEL_WPI if budget == 1 else _lib.TAB_KERNEL_WPI_INDEX), budget
        assert kw == (_lib.TAB_KERNEL_WPI if budget == 1 else _lib.TAB_KERNEL_PWG), budget
    for k, (a, b) in enumerate(zip(plain['shots'], pwg['shots'])):
        _same(a, b, 'launch %d' % k)
    last = plain['last']
    assert last['q'].any() and last['batches'] > 0 and last['lat_cnt'].sum() > 0
    return plain, pwg


def _mazes(side, seeds=(1234, 1235, 1236)):
    from cobel_amd.misc.gridworld_tools import make_obstacle_maze
    return [make_obstacle_maze(side, side, s) for s in seeds]


@pytest.mark.parametrize('side', SIDES)
def test_group_boundaries(side):
    """Budgets that are no multiple of four, three launches each: the launches start at every
    cp % 4, and each has a head and a tail of generic steps around its groups."""
    budgets = [130] + [b for b in (1, 2, 3, 4, 5, 7, 9, 130) for _ in range(3)]
    plain, _ = _both(_mazes(side), 40, budgets)
    from cobel_amd import _lib
    starts, cp = set(), 0
    for b in budgets:
        starts.add(cp & 3)
        cp += b
    assert starts == {0, 1, 2, 3}
    assert (plain['last']['inst'][:, _lib.I_CTR_POLICY] == cp).all()


def _goal_nearby(side):
    """An open field whose trials start one to three cells from the goal in its middle: trials of a
    few steps end at the goal as well as at the step limit, and the tables fill."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    mid = side // 2
    goal = mid * side + mid
    starts = [r * side + c for r in range(mid - 3, mid + 4) for c in range(mid - 3, mid + 4)
              if 1 <= abs(r - mid) + abs(c - mid) <= 3]
    return make_gridworld(side, side, terminals=[goal], rewards=np.array([[goal, 1.0]]),
                          goals=[goal], starting_states=starts)


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('spt', [3, 4, 5, 7])
def test_trial_ends_in_every_phase(side, spt):
    """Short trials end in every phase of a group; a small trials_target stops tickets inside one."""
    from cobel_amd import _lib
    n, target, budgets = 36, 9, [23, 50]
    plain, _ = _both([_goal_nearby(side)], n, budgets, spt=spt, trials_target=target, eps=0.3)
    inst = plain['last']['inst']
    trials = inst[:, _lib.I_TRIAL]
    steps = inst[:, _lib.I_STEPS_LO].astype(np.int64)
    assert plain['last']['lat_cnt'].sum() > 0            # trial ends were seen
    assert (trials == target).any()                       # somebody stopped at the target
    # an instance that reached the target ran exactly the steps of its `target` trials (latency
    # is the 0-based last step), the others the whole budget
    lat = plain['last']['lat_trace'].astype(np.int64)
    for i in range(n):
        if trials[i] == target:
            assert steps[i] == (lat[i, :target] + 1).sum(), i
        else:
            assert steps[i] == sum(budgets), i
    assert plain['last']['steps'] == steps.sum()
    ends = set()
    for i in range(n):
        done = np.cumsum(lat[i, :trials[i]] + 1)
        ends |= {int(d) & 3 for d in done}
    # (the policy counter at the trial ends)
    assert ends == {0, 1, 2, 3}


@pytest.mark.parametrize('side', SIDES)
def test_misaligned_counters_take_the_generic_loop(side):
    """Policy counters 1, 2 and 3 ahead of the memory counters for three quarters of the instances
    (what a call that draws from one stream alone leaves): no groups for them, same results."""
    from cobel_amd import _lib
    plain, _ = _both(_mazes(side), 40, [130, 9, 130], skew=(0, 1, 2, 3))
    inst = plain['last']['inst']
    apart = (inst[:, _lib.I_CTR_POLICY] - inst[:, _lib.I_CTR_MEMORY]) & 3
    assert np.array_equal(apart, np.arange(40) & 3)


@pytest.mark.parametrize('batch', [1, 50, 62])
def test_planning_widths_and_many_rounds(batch):
    """A small learning rate: most planning updates change their cell, many speculative rounds."""
    _both(_mazes(32, (77,)), 32, [150, 150], batch=batch, spt=40, alpha=0.5, eps=0.3)


def test_one_run_against_the_oracle():
    """Q of three instances against the NumPy reference loop driven by the same Philox streams."""
    from oracle import philox, ref_loop
    n, side, spt, batch, budgets = 24, 32, 40, 62, [150, 150]
    worlds = _mazes(side, (77,))
    out = _run(0, worlds, n, budgets, batch=batch, spt=spt, alpha=0.5, eps=0.3)
    from cobel_amd import _lib
    assert set(out['kinds']) == {_lib.TAB_KERNEL_PWG}
    tabs = worlds[0].compact()
    for i in (0, 7, 23):
        env = ref_loop.RefGridworld(tabs, philox.TapeRNG(SEED, i, philox.STREAM_ENV))
        pol = ref_loop.RefEpsilonGreedy(0.3, philox.TapeRNG(SEED, i, philox.STREAM_POLICY))
        ref = ref_loop.RefDynaQ(side * side, 4, pol, philox.TapeRNG(SEED, i, philox.STREAM_MEMORY),
                                dtype=np.float32, learning_rate=0.5)
        trials = int(out['last']['inst'][i, _lib.I_TRIAL])
        tr = ref_loop.new_trace()
        ref.train(env, trials, spt, batch, trace=tr)
        done = sum(s + 1 for s in tr['steps'])
        # the oracle runs whole trials: continue into the running one for the remaining steps
        left = sum(budgets) - done
        assert 0 <= left <= spt
        if left:
            ref.train(env, 1, left, batch, trace=tr)
        assert np.array_equal(out['last']['q'][i], ref.Q), i


def test_sliced_launches(monkeypatch):
    """Slices whose lengths are no multiples of four: a slice is a ticket with its own budget."""
    from cobel_amd import _lib
    # (a launch is sliced only when every CU has a workgroup: 256 x 10 wave slots)
    n, budgets, worlds = 2600, [67, 67], _mazes(32)
    plain = _run(_lib.F_NO_PWG, worlds, n, budgets, spt=30)
    monkeypatch.setenv('COBEL_DEBUG', '1')
    monkeypatch.setenv('COBEL_DEBUG_PWG_SLICES', '33,21,13')
    try:
        sliced = _run(0, worlds, n, budgets, spt=30)
    finally:
        monkeypatch.delenv('COBEL_DEBUG_PWG_SLICES', raising=False)
        monkeypatch.delenv('COBEL_DEBUG', raising=False)
    assert set(sliced['kinds']) == {_lib.TAB_KERNEL_PWG}
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    last = plain['last']
    assert last['q'].any() and last['batches'] > 0 and last['lat_cnt'].sum() > 0
    for k, (a, b) in enumerate(zip(plain['shots'], sliced['shots'])):
        _same(a, b, 'launch %d' % k)


def test_rewards_of_both_signs():
    """A positive and a negative terminal reward and a negative one on the way: the reward total of
    a trial is added to on rewarded steps only."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    side = 26
    goal, pit, toll = side * 13 + 13, side * 12 + 10, side * 13 + 11
    world = make_gridworld(side, side, terminals=[goal, pit],
                           rewards=np.array([[goal, 1.0], [pit, -1.0], [toll, -0.25]]),
                           goals=[goal],
                           starting_states=[side * 12 + 12, side * 13 + 10, side * 14 + 12,
                                            side * 11 + 10])
    plain, _ = _both([world], 40, [130, 131], spt=25, eps=0.3)
    last = plain['last']
    rs = last['reward_sum']
    assert (rs > 0).any()
    assert (rs < 0).any() or (rs != np.floor(rs)).any()   # (negative rewards were collected)
    assert 0 < last['resp_cnt'].sum() < last['lat_cnt'].sum()
