"""DQN on Continuous2D: milliseconds per lockstep step of ``DQN.train`` on the demo's open field
with its three obstacles (demo/continuous/demo_2d.py: tanh 64-64 network, batches of 32), for the
step robot and the wheel robot at 256 and 8 192 instances, in float64 and float32 — through the
two-kernel loop (cobel_dqn_act_c2d + cobel_dqn_replay) and with ``fused_loop = False``, the
PyTorch loop, which is the baseline: once as it runs now (its replay step is the tanh kernel
already) and once with ``fused_mlp = False`` as well — autograd for the network, the path a tanh
network took before the kernels existed.

The arena has no reward rows, so every trial lasts exactly ``--steps`` steps and a ``train()`` call
is ``trials * steps`` lockstep steps on both paths.  Per case both agents are built once and warmed
up with one call (library load, allocations, the recogniser's probes); then ``--repeats`` rounds
run the two paths alternately in this process, each timed call from a synchronised device to a
synchronised device — graph recording included, since every ``train()`` call pays it.  Prints one
JSON line per case: median, minimum and maximum of the rounds (docs/MEASUREMENTS.md §1).

    python scripts/bench_dqn_c2d.py [--trials 4] [--steps 64] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def arena():
    from cobel_amd.misc import continuous_tools as ct
    room = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    obstacles = [ct.make_rectangle(np.ones(2) / 2, 0.1, 0.1, 45),
                 ct.make_circle(np.array([0.9, 0.1]), 0.05),
                 ct.make_triangle(np.array([0.1, 0.9]), 0.1, 0.1)]
    return room, None, obstacles, np.zeros((0, 3))


def build(torch, robot, n, dtype, fused, ring):
    from cobel_amd.agent import DQN
    from cobel_amd.interface import Continuous2D
    from cobel_amd.memory import DQNMemory
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy
    n_in, n_out = (3, 3) if robot == 'wheel' else (2, 4)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layer_dense_1 = torch.nn.Linear(n_in, 64)
            self.layer_dense_2 = torch.nn.Linear(64, 64)
            self.layer_output = torch.nn.Linear(64, n_out)
            self.to(dtype)

        def forward(self, x):
            x = torch.tanh(self.layer_dense_1(x))
            x = torch.tanh(self.layer_dense_2(x))
            return self.layer_output(x)

    torch.manual_seed(1)
    env = Continuous2D(robot, *arena(), n_envs=n, seed=2024)
    agent = DQN(env.observation_space, env.action_space, EpsilonGreedy(0.3), TorchNetwork(Model()),
                0.9 ** 0.15, memory=DQNMemory(capacity=ring))
    agent.fused_loop = None if fused else False
    return agent, env


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--trials', type=int, default=4)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--instances', type=int, nargs='*', default=[256, 8192])
    args = ap.parse_args()
    import torch
    per_call = args.trials * args.steps

    def timed(agent, env):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.train(env, args.trials, args.steps, 32)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / per_call

    for dtype in (torch.float64, torch.float32):
        for robot in ('step', 'wheel'):
            for n in args.instances:
                # torch_loop: fused_loop = False on this code — the bookkeeping in PyTorch, the replay
                # step already cobel_dqn_replay with tanh; torch_loop_autograd: the same with
                # fused_mlp = False, i.e. forward / backward by autograd and the fused Adam kernel,
                # which is what a tanh network ran on before the activation selector existed
                pair = {name: build(torch, robot, n, dtype, name == 'fused', per_call)
                        for name in ('fused', 'torch_loop', 'torch_loop_autograd')}
                for name in pair:
                    timed(*pair[name])                       # warm-up
                auto = pair['torch_loop_autograd'][0]
                auto._online.fused_mlp = auto._target.fused_mlp = False
                timed(*pair['torch_loop_autograd'])          # (warm-up of the autograd step)
                ms = {name: [] for name in pair}
                for _ in range(args.repeats):
                    for name in pair:
                        ms[name].append(timed(*pair[name]))
                fused_agent, loop_agent = pair['fused'][0], pair['torch_loop'][0]
                # (the loop counts launches: a call may end with a chunk in which nobody steps any more)
                assert fused_agent.fused_steps >= per_call * (args.repeats + 1), fused_agent.fused_steps
                assert int(fused_agent.trial.min()) == int(loop_agent.trial.min()) \
                    == args.trials * (args.repeats + 1)
                assert loop_agent.fused_steps == 0 and auto.fused_steps == 0
                out = {'bench': 'dqn_c2d', 'robot': robot, 'instances': n,
                       'dtype': str(dtype).split('.')[-1], 'lockstep_steps_per_call': per_call,
                       'repeats': args.repeats}
                for name, v in ms.items():
                    v = sorted(v)
                    out[name + '_ms_per_step'] = {'median': round(v[len(v) // 2], 4),
                                                  'min': round(v[0], 4), 'max': round(v[-1], 4)}
                for name in ('torch_loop', 'torch_loop_autograd'):
                    out[name + '_over_fused'] = round(
                        out[name + '_ms_per_step']['median'] / out['fused_ms_per_step']['median'], 2)
                print(json.dumps(out), flush=True)
                del pair


if __name__ == '__main__':
    main()
