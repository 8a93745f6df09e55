#!/usr/bin/env python3
"""Env-steps/s of DynaQ and QAgent with a Softmax policy (cobel_tab_policy_run, csrc/tabular_policy.hip)
at 65 536 instances on the 32 x 32 open field, planning / replay batch 50 / 32, next to the
epsilon-greedy run of the same shape on cobel_tab_run's kernels.  One untimed session, then five
timed ones (host clock around a session that ends in a device synchronise); prints the median and
the minimum time per leg and one JSON line.  docs/MEASUREMENTS.md section 32 holds the figures.

    python scripts/bench_tabpol.py [--instances 65536] [--trials 2] [--steps 64] [--sessions 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def leg(torch, agent_name, policy_name, args):
    from cobel_amd.agent import DynaQ, QAgent
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_open_field
    from cobel_amd.policy import EpsilonGreedy, Softmax
    env = Gridworld(make_open_field(32, 32, 0, 1), n_envs=args.instances, seed=2024)
    policy = Softmax(2.0) if policy_name == 'softmax' else EpsilonGreedy(0.1)
    cls, batch = (DynaQ, 50) if agent_name == 'dynaq' else (QAgent, 32)
    ag = cls(env.observation_space, env.action_space, policy)
    if agent_name == 'q':
        ag.log_experiences = True
    times, steps = [], []
    for k in range(args.sessions + 1):
        before = ag.env_steps()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ag.train(env, args.trials, args.steps, batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if k:       # (the first session is the warm-up)
            times.append(dt)
            steps.append(ag.env_steps() - before)
    rates = [s / t for s, t in zip(steps, times)]
    return {'agent': agent_name, 'policy': policy_name, 'batch': batch,
            'steps_per_session': int(statistics.median(steps)),
            'median_s': statistics.median(times), 'min_s': min(times),
            'median_steps_per_s': statistics.median(rates), 'max_steps_per_s': max(rates)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=65536)
    ap.add_argument('--trials', type=int, default=2)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--sessions', type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_tabpol.py needs a GPU'
    out = []
    for agent_name in ('dynaq', 'q'):
        for policy_name in ('softmax', 'eps_greedy'):
            r = leg(torch, agent_name, policy_name, args)
            out.append(r)
            print('%-6s %-10s batch %2d: median %.4f s, min %.4f s, %.3e env-steps/s (median), '
                  '%.3e (best)' % (r['agent'], r['policy'], r['batch'], r['median_s'], r['min_s'],
                                   r['median_steps_per_s'], r['max_steps_per_s']), flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({'bench': 'tabpol', 'instances': args.instances, 'trials': args.trials,
                      'steps': args.steps, 'legs': out}))


if __name__ == '__main__':
    main()
