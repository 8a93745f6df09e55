"""Times QAgent on a Sequence in the grid-search demo's configuration: four one-hot stimuli, eight
arms, 400 single-step trials, batches of 32 replayed experiences per step, a softmax policy with
per-instance learning rate and beta — at 2 700 instances (the demo's 27 combinations x 100 runs) and
at 65 536.  One untimed session, then five timed ones (fresh agent and environment each, the host
clock around a device synchronisation); prints the median and the minimum, env-steps/s and replay
updates/s, and the same for the NumPy restatement of tests/qseq_common.py on one host core.

    python scripts/bench_qseq.py [--instances 2700 65536] [--trials 400] [--batch 32] [--host 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')]


def design(trials: int):
    names = 'ABCD'
    seq = [[{'observation': names[t % 4], 'reward': np.eye(8)[2 * (t % 4)], 'action': None}]
           for t in range(trials)]
    return seq, {n: np.eye(4)[k] for k, n in enumerate(names)}


def device(n: int, trials: int, batch: int, repeats: int) -> dict:
    import torch
    from cobel_amd.agent import QAgent
    from cobel_amd.interface import Sequence
    from cobel_amd.policy import Softmax
    from cobel_amd.spaces import Box
    seq, obs = design(trials)
    rng = np.random.default_rng(0)
    lr = rng.choice(np.arange(1, 10) / 10, n)
    beta = rng.choice([1.0, 5.0, 10.0], n)
    times = []
    for r in range(repeats + 1):
        env = Sequence(seq, obs, Box(0.0, 1.0, (4,)), 8, n_envs=n, seed=7)
        ag = QAgent(env.observation_space, env.action_space, Softmax(beta), learning_rate=lr)
        ag.train(env, 0, 100, batch)          # (binds and allocates; nothing is launched)
        ag._seq.reserve_replay(trials)
        ag._seq._reserve(trials)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ag.train(env, trials, 100, batch)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        assert ag.env_steps() == n * trials
    times = np.array(times[1:])
    med, best = float(np.median(times)), float(times.min())
    return {'instances': n, 'trials': trials, 'batch': batch, 'median_s': med, 'min_s': best,
            'env_steps_per_s': n * trials / med, 'updates_per_s': n * trials * (batch + 1) / med}


def host(n: int, trials: int, batch: int) -> dict:
    import qseq_common as qc
    seq, obs = design(trials)
    t0 = time.perf_counter()
    for i in range(n):
        qc.restate(seq, obs, 8, False, ('softmax', 1.0), None, 0.9, 0.8, [('train', trials, 100, batch)], i)
    dt = time.perf_counter() - t0
    return {'host_instances': n, 'host_s': dt, 'host_env_steps_per_s': n * trials / dt,
            'host_updates_per_s': n * trials * (batch + 1) / dt}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--instances', type=int, nargs='+', default=[2700, 65536])
    ap.add_argument('--trials', type=int, default=400)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host', type=int, default=2, help='instances of the restatement to time (0: none)')
    args = ap.parse_args()
    for n in args.instances:
        print(json.dumps(device(n, args.trials, args.batch, args.repeats)))
    if args.host:
        print(json.dumps(host(args.host, args.trials, args.batch)))


if __name__ == '__main__':
    main()
