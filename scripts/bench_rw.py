"""Rescorla-Wagner throughput: the configuration of demo/sequence/demo_rw_binary.py (four one-hot
stimuli, 1 000 single-step trials, Sigmoid(scale=1.0), W filled with 0.5, half of the trials
trained, half tested) at 65 536 instances, against the restatement of tests/rw_common.py on one
host core.  Prints one JSON line.  No target is set: the kernel is untuned.

    python scripts/bench_rw.py [--n 65536] [--repeats 5]
"""
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
import rw_common as rc  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    import torch
    schedule, obs = rc.demo_design(250)
    trials = len(schedule)
    sessions = [('train', trials // 2, 100), ('test', trials - trials // 2, 100)]
    policy = ('sigmoid', dict(scale=1.0))

    def device_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ag, env = rc.device_run(schedule, obs, 2, False, policy, None, 0.9, sessions, n_envs=args.n,
                                w0=0.5, record=0)
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
        return ag, whole

    def launches_once(ag_env):
        """The two launches alone, on a bound agent and a fresh Sequence."""
        from cobel_amd.interface import Sequence
        ag = ag_env
        env = Sequence(schedule, obs, ag.observation_space, 2, n_envs=args.n, seed=rc.SEED)
        ag.W.fill(0.5)
        ag.current_trial = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ag.train(env, sessions[0][1], 100)
        ag.test(env, sessions[1][1], 100)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ag, _ = device_once()               # warm-up: library load, allocations
    whole = sorted(device_once()[1] for _ in range(args.repeats))
    launch = sorted(launches_once(ag) for _ in range(args.repeats))
    steps = args.n * trials
    t0 = time.perf_counter()
    ref = rc.restate(schedule, obs, 2, False, policy, None, 0.9, sessions, 0, 0.5)
    host = time.perf_counter() - t0
    print(json.dumps({
        'bench': 'rw_binary_demo', 'instances': args.n, 'trials': trials, 'env_steps': steps,
        'device_seconds_median': launch[len(launch) // 2], 'device_seconds_min': launch[0],
        'device_env_steps_per_s': steps / launch[len(launch) // 2],
        'with_setup_seconds_median': whole[len(whole) // 2],
        'host_restatement_env_steps_per_s': len(ref['value']) / host,
        'speedup_vs_one_core_restatement': (steps / launch[len(launch) // 2]) / (len(ref['value']) / host),
        'repeats': args.repeats}))


if __name__ == '__main__':
    main()
