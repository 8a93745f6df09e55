"""DQN.train on Continuous2D with the demo's tanh 64-64 model and batches of 32 through the
two-kernel loop (cobel_dqn_act_c2d + cobel_dqn_replay with activation = tanh, recorded into a HIP
graph) against the PyTorch loop it replaces (``fused_loop = False``): device against device, so the
wheel robot is exact too.  Six instances with an instance_base, 3 trials of at most 12 steps on the
demo's open field with reward rows placed so that some trials end early, a ring of 20 rows that
wraps, and a second train() call that continues.

Identical: the rings, env_ctr, the policy and memory counters, trial counts, monitors and
reset_fallbacks.  ``env.state`` is compared in the instances that took part in the last lockstep
step: an instance that has run its trials is frozen by the fused kernels (nothing of its own is
written), while the PyTorch loop goes on stepping its environment, masked out of everything else.
Weights and moments: rtol 1e-9 / atol 1e-12 in float64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c2d_common as cc  # noqa: E402

pytestmark = pytest.mark.gpu

REWARDS = np.array([[0.25, 0.25, 10.0], [0.75, 0.75, 8.0], [0.25, 0.75, 6.0], [0.75, 0.25, 4.0],
                    [0.5, 0.2, 3.0], [0.5, 0.8, 2.0], [0.2, 0.5, 1.0], [0.8, 0.5, 0.5]])


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


def _arena():
    from cobel_amd.misc import continuous_tools as ct
    room = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    obstacles = [ct.make_rectangle(np.ones(2) / 2, 0.1, 0.1, 45), ct.make_circle(np.array([0.9, 0.1]), 0.05),
                 ct.make_triangle(np.array([0.1, 0.9]), 0.1, 0.1)]
    return room, None, obstacles, REWARDS.copy()


def _model(torch, n_in, n_out, act, dtype):
    class Model(torch.nn.Module):        # the demo's model: a custom forward
        def __init__(self):
            super().__init__()
            self.layer_dense_1 = torch.nn.Linear(n_in, 64)
            self.layer_dense_2 = torch.nn.Linear(64, 64)
            self.layer_output = torch.nn.Linear(64, n_out)
            self.to(dtype)

        def forward(self, x):
            x = act(self.layer_dense_1(x))
            x = act(self.layer_dense_2(x))
            return self.layer_output(x)
    return Model()


def _run(torch, robot, fused, act=None, dtype=None, batch=32, fused_loop=None, calls=((3, 12), (2, 12))):
    from cobel_amd.agent import DQN
    from cobel_amd.interface import Continuous2D
    from cobel_amd.memory import DQNMemory
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy
    torch.manual_seed(7)
    env = Continuous2D(robot, *_arena(), n_envs=6, seed=99, instance_base=21)
    n_in, n_out = (3, 3) if robot == 'wheel' else (2, 4)
    net = _model(torch, n_in, n_out, act or torch.tanh, dtype or torch.float64)
    ag = DQN(env.observation_space, env.action_space, EpsilonGreedy(0.3), TorchNetwork(net),
             gamma=0.9, memory=DQNMemory(capacity=20))
    ag.fused_loop = fused_loop if fused else False
    ag.use_graph = None if fused else False
    for trials, steps in calls:
        ag.train(env, trials, steps, batch)
    torch.cuda.synchronize()
    return ag, env


def _same_run(torch, a, ea, b, eb, trials):
    assert torch.equal(a.trial, b.trial) and int(a.trial.min()) == trials
    for k in ('lat_sum', 'lat_cnt', 'reward_sum'):
        assert torch.equal(getattr(a.monitors, k), getattr(b.monitors, k)), k
    for x, y in ((a.M.size, b.M.size), (a.M.head, b.M.head), (a.M.actions, b.M.actions),
                 (a.M.rewards, b.M.rewards), (a.M.states, b.M.states),
                 (a.M.next_states, b.M.next_states), (a.M.terminals, b.M.terminals),
                 (a.M.counter, b.M.counter), (a.policy.counter, b.policy.counter)):
        assert torch.equal(x, y)
    for i in range(6):
        for x, y in zip(a._online.get_weights(i) + a._target.get_weights(i),
                        b._online.get_weights(i) + b._target.get_weights(i)):
            assert np.allclose(x, y, rtol=1e-9, atol=1e-12), float(np.abs(x - y).max())
    for (k, x), y in zip(a._online.params.items(), b._online.params.values()):
        sx, sy = a._online.optimizer.state[x], b._online.optimizer.state[y]
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.allclose(sx[key], sy[key], rtol=1e-9, atol=1e-12), (k, key)
        assert torch.equal(sx['steps'], sy['steps'])
    assert a.current_trial == b.current_trial == trials


@pytest.mark.parametrize('robot', ['step', 'wheel'])
def test_fused_loop_equals_torch_loop_on_the_arena(torch_cuda, robot):
    torch = torch_cuda
    (a, ea), (b, eb) = _run(torch, robot, True), _run(torch, robot, False)
    # (trials of 12 steps are launched directly: the loop records its graph from 16 steps on)
    assert a.fused_steps > 0 and b.fused_steps == 0 and a.fused_graph_steps == 0
    _same_run(torch, a, ea, b, eb, 5)
    assert torch.equal(ea.env_ctr, eb.env_ctr) and ea.reset_fallbacks == eb.reset_fallbacks == 0
    last = a._fused_keep[-1].bool()                 # `stepped` of the last lockstep step
    assert bool(last.any()) and torch.equal(ea.state[last], eb.state[last])
    assert torch.equal(ea.wall_hit[last], eb.wall_hit[last])
    # the ring wrapped somewhere, and some trial ended before its step limit
    assert int(a.M.size.max()) == 20 and int(a.M.head.max()) > 0
    cnt, lat = a.monitors.lat_cnt[:5].sum(), a.monitors.lat_sum[:5].sum()
    assert int(cnt) == 30 and int(lat) < 30 * 11
    if robot == 'step':     # every stored transition is one restatement step
        M = a.M
        s, act, r = M.states.cpu().numpy(), M.actions.cpu().numpy(), M.rewards.cpu().numpy()
        ns, nt, size = M.next_states.cpu().numpy(), M.terminals.cpu().numpy(), M.size.cpu().numpy()
        T = ea.geometry['edges']
        for i in range(6):
            for k in range(size[i]):
                ws, wr, wd, _ = cc.step(T, ea.R, cc.STEP, (s[i, k, 0], s[i, k, 1], 0.0), int(act[i, k]))
                assert ns[i, k].tolist() == list(ws[:2]) and r[i, k] == wr and nt[i, k] == 1.0 - wd, (i, k)


def test_fused_loop_replayed_from_its_graph(torch_cuda):
    """Trials of at most 16 steps: the two launches are recorded once, 16 steps to a graph, and
    replayed (frozen instances are skipped inside it) — the same run as the PyTorch loop's."""
    torch = torch_cuda
    calls = ((3, 16), (2, 16))
    (a, ea), (b, eb) = _run(torch, 'step', True, calls=calls), _run(torch, 'step', False, calls=calls)
    assert a.fused_steps > 0 and a.fused_graph_steps > 0 and b.fused_steps == 0
    _same_run(torch, a, ea, b, eb, 5)
    assert torch.equal(ea.env_ctr, eb.env_ctr) and ea.reset_fallbacks == eb.reset_fallbacks


def test_float32_runs_to_the_same_trial_counts(torch_cuda):
    torch = torch_cuda
    a, ea = _run(torch, 'step', True, dtype=torch.float32)
    assert a.fused_steps > 0 and a.trial.tolist() == [5] * 6
    assert all(bool(torch.isfinite(p).all()) for p in a._online.params.values())
    assert all(bool(torch.isfinite(p).all()) for p in a._target.params.values())


def test_relu_model_on_the_arena(torch_cuda):
    torch = torch_cuda
    (a, ea), (b, eb) = _run(torch, 'step', True, act=torch.relu), _run(torch, 'step', False, act=torch.relu)
    assert a.fused_steps > 0 and b.fused_steps == 0
    _same_run(torch, a, ea, b, eb, 5)
    assert torch.equal(ea.env_ctr, eb.env_ctr)


def test_tanh_model_on_a_topology(torch_cuda):
    """The activation selector alone: a tanh model on linear_track(10, 2) takes the two-kernel loop
    of cobel_dqn_act + cobel_dqn_replay and matches its PyTorch loop."""
    torch = torch_cuda
    from cobel_amd.agent import DQN
    from cobel_amd.interface import Topology
    from cobel_amd.memory import DQNMemory
    from cobel_amd.misc.topology_tools import linear_track
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy
    nodes, starts = linear_track(10, 2)

    def run(fused):
        torch.manual_seed(5)
        env = Topology(nodes, starts, n_envs=6, seed=31, instance_base=4)
        net = _model(torch, int(env.observation_space.shape[0]), int(env.action_space.n), torch.tanh,
                     torch.float64)
        ag = DQN(env.observation_space, env.action_space, EpsilonGreedy(0.4), TorchNetwork(net),
                 gamma=0.8, memory=DQNMemory(capacity=20))
        ag.fused_loop = None if fused else False
        ag.use_graph = None if fused else False
        ag.train(env, 3, 12, 32)
        ag.train(env, 2, 12, 32)
        torch.cuda.synchronize()
        return ag, env

    (a, ea), (b, eb) = run(True), run(False)
    assert a.fused_steps > 0 and b.fused_steps == 0
    _same_run(torch, a, ea, b, eb, 5)
    assert torch.equal(ea.env_ctr, eb.env_ctr)


def test_routes_that_stay_on_the_torch_loop(torch_cuda):
    """Batches of 8, a hardtanh model and fused_loop = False."""
    torch = torch_cuda
    one = ((2, 6),)
    assert _run(torch, 'step', True, batch=8, calls=one)[0].fused_steps == 0
    assert _run(torch, 'step', True, act=torch.nn.functional.hardtanh, calls=one)[0].fused_steps == 0
    assert _run(torch, 'step', True, fused_loop=False, calls=one)[0].fused_steps == 0
    assert _run(torch, 'step', True, calls=one)[0].fused_steps > 0
