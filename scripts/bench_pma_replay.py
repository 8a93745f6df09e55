#!/usr/bin/env python3
"""PMAMemory.replay / update_sr and PMA.train on one MI355X: replay rounds/s of `replay(32)` on the
demo's 5 x 5 world and on an 11 x 11 world at `--instances` instances (memories filled by a few
trials of training first), `update_sr` calls/s (instances x calls), and trials/s of the demo
configuration (mask_actions, gamma_q 0.99, batch 32, 50 steps).

Method (docs/MEASUREMENTS.md): one process, the GPU warmed by the training and one untimed call;
`--windows` windows of `--calls` device calls each between two HIP events on the calls' stream, no
host synchronisation inside a window; median window, slowest and fastest beside it.  The replay
is timed on the device call alone (`PMAMemory._replay_device`: the records stay on the device).
The comparison is the NumPy restatement (tests/pma_common.py) doing the same on one host core.

    python scripts/bench_pma_replay.py [--instances 16384] [--length 32] [--worlds 5x5,11x11]

Prints one JSON line per world."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 2024


def world_of(name):
    import pma_common as pc
    h, w = (int(x) for x in name.split('x'))
    return pc.demo_world() if (h, w) == (5, 5) else pc.seeded_world(h, w, seed=h)


def build(world, n):
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(world, n_envs=n, seed=SEED)
    mem = PMAMemory(env.world['sas'], EpsilonGreedy(0.1), gamma_q=0.99)
    agent = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    agent.mask_actions = True
    return env, agent, mem


def windows_of(torch, fn, windows, calls):
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def host_rates(world, length, trials):
    import pma_common as pc
    tabs, sas = pc.tables_of(world)
    env, agent, mem = pc.make_ref_agent(tabs, sas, SEED, 0)
    agent.mask_actions = True
    t0 = time.perf_counter()
    agent.train(env, trials, 50, length)
    t_train = time.perf_counter() - t0
    start = int(tabs['starts'][0])
    t0 = time.perf_counter()
    mem.replay(agent.Q, agent.action_mask, length, start)
    t_replay = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(20):
        mem.update_sr()
    t_sr = (time.perf_counter() - t0) / 20
    return length / t_replay, 1.0 / t_sr, trials / t_train


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=16384)
    ap.add_argument('--length', type=int, default=32)
    ap.add_argument('--worlds', default='5x5,11x11')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--warm-trials', type=int, default=3)
    ap.add_argument('--host-trials', type=int, default=3)
    a = ap.parse_args()
    import torch
    for name in a.worlds.split(','):
        world = world_of(name)
        n, L = a.instances, a.length
        env, agent, mem = build(world, n)
        agent.train(env, a.warm_trials, 50, L)
        torch.cuda.synchronize()
        start = np.full(n, int(world['starting_states'][0]), dtype=np.int32)
        bits = agent._mask_bits()
        q = agent._q.clone()
        fn = lambda: mem._replay_device(q, bits, L, start, None, None)      # noqa: E731
        fn()
        rep = windows_of(torch, fn, a.windows, a.calls)
        mem.update_sr()
        sr = windows_of(torch, mem.update_sr, a.windows, a.calls)
        out = {'world': name, 'instances': n, 'replay_length': L, 'plan': mem.launch_plan(L),
               'replay_ms': [round(x / a.calls, 4) for x in rep],
               'replay_rounds_per_s': n * L * a.calls / (rep[0] * 1e-3),
               'update_sr_ms': [round(x / a.calls, 4) for x in sr],
               'update_sr_per_s': n * a.calls / (sr[0] * 1e-3)}
        if name == '5x5':
            t0 = time.perf_counter()
            agent.train(env, 5, 50, L)
            torch.cuda.synchronize()
            out['train_trials_per_s'] = n * 5 / (time.perf_counter() - t0)
        h = host_rates(world, L, a.host_trials)
        out.update({'host_replay_rounds_per_s': h[0], 'host_update_sr_per_s': h[1],
                    'host_train_trials_per_s': h[2]})
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
