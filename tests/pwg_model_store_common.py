"""Helpers of tests/test_gpu_pwg_model_store.py: the launch-by-launch driver of
tests/pwg_trial_ends_common.py with the memory's learning rate as an argument, a comparison of two
runs byte for byte (NaN reward estimates included), and the worlds the cases use."""
import numpy as np
import torch

from conftest import SEED
from pwg_trial_ends_common import KEYS, NO_TARGET, snapshot


def run(extra_flags, make_worlds, n, launches, batch=50, spt=60, alpha=0.99, eps=0.1, model_lr=None,
        between=None):
    """One agent on `make_worlds()`, one launch per entry of `launches` (a step budget), a snapshot
    after every launch.  `between`: {k: f(env)} — f edits the worlds in place before launch k; the
    edit is pushed to the device (the live-world path)."""
    from cobel_amd import _lib
    from cobel_amd.agent import DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(make_worlds(), n_envs=n, seed=SEED, device=torch.device('cuda', 0))
    agent = DynaQ(env.observation_space, env.action_space, EpsilonGreedy(eps), learning_rate=alpha)
    if model_lr is not None:
        agent.M.learning_rate = model_lr
    agent.extra_flags = extra_flags
    agent.track_instances = True
    agent.track_responses = True
    agent._bind(env)
    agent._env_in(env)
    flags = _lib.F_LEARN | agent._policy_in(agent.policy, env, False)
    agent.monitors.reserve(2048, n, True)
    kinds, shots = [], []
    for k, budget in enumerate(launches):
        if between and k in between:
            between[k](env)
            assert env.sync_world() is True
        kinds.append(agent.describe_launch(env, agent.policy, flags, NO_TARGET, spt, budget,
                                           batch)['kernel'])
        agent._launch(env, agent.policy, flags, NO_TARGET, spt, budget, batch)
        torch.cuda.synchronize()
        shots.append(snapshot(agent))
    return {'kinds': kinds, 'shots': shots, 'last': shots[-1]}


def same(a, b, where=''):
    """Bit for bit: a NaN reward estimate (and what planning makes of it in Q) must be the same NaN."""
    for key in KEYS:
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (key, where)
    assert a['batches'] == b['batches'] and a['steps'] == b['steps'], where


def both(make_worlds, n, launches, pwg_flags=0, planned=True, **args):
    """The wave-per-instance kernel, which stores the model record in every step, and the persistent
    one on the same inputs: equal after every launch.  Returns the reference's run.  `planned`: some
    instance must have found a reward, so that planning batches ran (they read what the step stores
    or skips)."""
    from cobel_amd import _lib
    plain = run(_lib.F_NO_PWG, make_worlds, n, launches, **args)
    pwg = run(pwg_flags, make_worlds, n, launches, **args)
    assert set(plain['kinds']) == {_lib.TAB_KERNEL_WPI_INDEX}
    assert set(pwg['kinds']) == {_lib.TAB_KERNEL_PWG}
    for k, (a, b) in enumerate(zip(plain['shots'], pwg['shots'])):
        same(a, b, 'launch %d' % k)
    assert plain['last']['batches'] > 0 or not planned
    return plain


def unpack(shot):
    """(reward estimate bits, successor, non-terminal bit) of every model record, and the digest."""
    raw = shot['model'].astype(np.uint64).reshape(shot['model'].shape[0], -1)
    return ((raw & np.uint64(0xffffffff)).astype(np.uint32), ((raw >> np.uint64(32)) & np.uint64(0xffff)).astype(np.int64),
            ((raw >> np.uint64(48)) & np.uint64(1)).astype(np.int64),
            shot['index'].astype(np.int64).reshape(shot['index'].shape[0], -1) & 0xffff)


def one_maze(side, goal=0):
    """The benchmark's obstacle maze; `goal`: the rewarded terminal (the corner, as in the benchmark —
    fresh agents do not find it in two trials — or a cell in the middle, which some do)."""
    from cobel_amd.misc.gridworld_tools import make_obstacle_maze
    return lambda: [make_obstacle_maze(side, side, 1234, goal_state=goal)]


def cell_and_goal(side):
    """Two starts: a cell walled in on all four sides (every action bumps: the same state, and
    every fourth step on average the same pair as the step before), and a cell two steps from a
    rewarded terminal (so that the tables fill and planning runs)."""
    from cobel_amd.misc.gridworld_tools import make_gridworld
    mid = side // 2
    cell = 3 * side + 3
    goal = mid * side + mid
    walls = [(cell, cell + d) for d in (-1, 1, -side, side)]
    return lambda: [make_gridworld(side, side, terminals=[goal], rewards=np.array([[goal, 1.0]]),
                                   goals=[goal], starting_states=[cell, goal - 2],
                                   invalid_transitions=walls)]
