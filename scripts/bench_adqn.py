"""ADQN throughput: the design of unit_tests/test_adqn.py (two one-hot stimuli, A rewarded, B
punished, single-step trials) with a Linear(2, 64)-ReLU-Linear(64, 64)-ReLU-Linear(64, 1) network
in float64, batches of 32 and one replay per step — the fused path, 1 + 1 launches per lockstep
step — at 4 096 instances, against the restatement of tests/adqn_common.py on one host core.
Prints one JSON line.  No target is set: store and scan are O(count) per step and untuned.

    python scripts/bench_adqn.py [--n 4096] [--trials 200] [--repeats 3]
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
import adqn_common as ac  # noqa: E402
import mlp_common as mc  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--trials', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    import torch
    schedule, obs, seq_actions = ac._unit()
    schedule = (schedule * (args.trials // len(schedule) + 1))[:args.trials]
    params = mc.one(mc.draw_networks(np.random.default_rng(1), 1, 2, 1, np.float64), 0)
    sessions = [('train', args.trials, 10, 32, 1)]

    def device_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ag, _ = ac.device_run(schedule, obs, False, seq_actions, params, 0.9, True, sessions,
                              n_envs=args.n, record=0)
        torch.cuda.synchronize()
        assert ag.fused_steps == args.trials and ag.env_steps() == args.n * args.trials
        return time.perf_counter() - t0

    device_once()               # warm-up: library load, allocations
    whole = sorted(device_once() for _ in range(args.repeats))
    steps = args.n * args.trials
    short = min(args.trials, 100)
    t0 = time.perf_counter()
    ac.restate(schedule, obs, False, seq_actions, params, 0.9, True, [('train', short, 10, 32, 1)],
               0, 32)
    host = time.perf_counter() - t0
    print(json.dumps({
        'bench': 'adqn_unit_design', 'instances': args.n, 'trials': args.trials, 'env_steps': steps,
        'batch_size': 32, 'nb_replays': 1, 'dtype': 'float64',
        'session_seconds_median': whole[len(whole) // 2], 'session_seconds_min': whole[0],
        'device_env_steps_per_s': steps / whole[len(whole) // 2],
        'host_restatement_env_steps_per_s': short / host,
        'speedup_vs_one_core_restatement': (steps / whole[len(whole) // 2]) / (short / host),
        'repeats': args.repeats}))


if __name__ == '__main__':
    main()
