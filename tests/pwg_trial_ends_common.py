"""Helpers of tests/test_gpu_pwg_trial_ends.py: one agent driven launch by launch through the
low-level launch call, a snapshot of everything the kernels leave after every launch, and the
worlds the cases use."""
import numpy as np
import torch

from conftest import SEED

KEYS = ('q', 'model', 'index', 'inst', 'lat_sum', 'lat_cnt', 'reward_sum', 'resp_cnt', 'lat_trace')
NO_TARGET = 0x7fffffff


def snapshot(agent):
    mon = agent.monitors
    out = {'q': agent._q, 'model': agent.M.table, 'index': agent.M.index, 'inst': agent.inst,
           'lat_sum': mon.lat_sum, 'lat_cnt': mon.lat_cnt, 'reward_sum': mon.reward_sum,
           'resp_cnt': mon.resp_cnt, 'lat_trace': mon.lat_trace}
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out['batches'] = int(agent.batches_done.item())
    out['steps'] = agent.env_steps()
    return out


def run(extra_flags, make_worlds, n, launches, batch=50, spt=60, alpha=0.99, eps=0.1, skew=None,
        between=None):
    """One agent on `make_worlds()`, one launch per entry of `launches` — a step budget, or
    (budget, trials_target) —, a snapshot after every launch.  `skew`: added to the policy counter of
    instance i before the first launch (skew[i % len(skew)]).  `between`: {k: f(env)} — f edits the
    worlds before launch k; the edit is pushed to the device."""
    from cobel_amd import _lib
    from cobel_amd.agent import DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(make_worlds(), n_envs=n, seed=SEED, device=torch.device('cuda', 0))
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
    start = agent.inst.cpu().numpy().copy()   # the instance records before the first launch
    kinds, shots = [], []
    for k, launch in enumerate(launches):
        budget, target = launch if isinstance(launch, tuple) else (launch, NO_TARGET)
        if between and k in between:
            between[k](env)
            assert env.sync_world() is True
        kinds.append(agent.describe_launch(env, agent.policy, flags, target, spt, budget,
                                           batch)['kernel'])
        agent._launch(env, agent.policy, flags, target, spt, budget, batch)
        torch.cuda.synchronize()
        shots.append(snapshot(agent))
    return {'kinds': kinds, 'shots': shots, 'last': shots[-1], 'start': start}


def same(a, b, where=''):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (key, where)
    assert a['batches'] == b['batches'] and a['steps'] == b['steps'], where


def both(make_worlds, n, launches, **args):
    """The wave-per-instance kernel (the reference) and the persistent one on the same inputs,
    equal after every launch.  Returns the reference's run."""
    from cobel_amd import _lib
    plain = run(_lib.F_NO_PWG, make_worlds, n, launches, **args)
    pwg = run(0, make_worlds, n, launches, **args)
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    assert set(pwg['kinds']) == {_lib.TAB_KERNEL_PWG}
    for k, (a, b) in enumerate(zip(plain['shots'], pwg['shots'])):
        same(a, b, 'launch %d' % k)
    last = plain['last']
    assert last['q'].any() and last['batches'] > 0 and last['lat_cnt'].sum() > 0
    return plain


def mazes(side, seeds=(1234, 1235, 1236)):
    from cobel_amd.misc.gridworld_tools import make_obstacle_maze
    return [make_obstacle_maze(side, side, s) for s in seeds]


def goal_field(side, starts, shift=0):
    """An open field with the goal `shift` cells right of its middle and the given start list."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    mid = side // 2
    goal = mid * side + mid + shift
    return make_gridworld(side, side, terminals=[goal], rewards=np.array([[goal, 1.0]]),
                          goals=[goal], starting_states=list(starts))


def goal_nearby(side, shift=0):
    """Trials start one to three cells from the goal: trials of a few steps end at the goal as well
    as at the step limit."""
    mid = side // 2
    starts = [r * side + c + shift for r in range(mid - 3, mid + 4) for c in range(mid - 3, mid + 4)
              if 1 <= abs(r - mid) + abs(c - mid) <= 3]
    return goal_field(side, starts, shift)
