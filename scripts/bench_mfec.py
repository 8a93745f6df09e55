#!/usr/bin/env python3
"""MFEC.train on one MI355X: env-steps/s of the configuration of demo/topology/demo_mfec.py — the
linear track with one-hot observations, k 10, capacity 2 000, epsilon 1e-4, 500 trials of 50 steps —
at 1, 1 024 and 16 384 instances (`--instances`).

Method (docs/MEASUREMENTS.md section 1): one process; per instance count a fresh agent, one untimed
session of `--warm-trials` trials (allocations, first launches, the pair tables), then ONE timed
`train()` of `--trials` trials — a single launch — between two HIP events on its stream; steps are
the kernels' own count (`agent.env_steps()`), so trials that end early count what they ran.  With
`--repeats` the timed session runs again on the grown memories: the later, slower sessions are
reported beside the first (the scan grows with the buffers).  The host comparison is the NumPy
restatement (tests/mfec_common.py) on one core over `--host-trials` trials and, where
COBEL_REFERENCE_SRC names a checkout and scikit-learn is installed, the reference itself.

    python scripts/bench_mfec.py [--instances 1,1024,16384] [--trials 500] [--host-trials 60]

Prints one JSON line per instance count, then one for the host."""
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
K, CAPACITY, EPSILON, STEPS = 10, 2000, 0.0001, 50


def make(n):
    from cobel_amd.agent import MFEC
    from cobel_amd.interface import Topology
    from cobel_amd.interface.simulator.offline import OfflineSimulator
    from cobel_amd.misc.topology_tools import linear_track
    from cobel_amd.policy import EpsilonGreedy
    from cobel_amd.spaces import Box
    nodes, starts = linear_track(10, 2, 1.0, 20, 'right')
    S = len(nodes)
    obs = {tuple(nodes[k]['pose']): o for k, o in zip(nodes, np.eye(S))}
    env = Topology(nodes, starts, OfflineSimulator(obs, Box(0.0, 1.0, (S,))), n_envs=n, seed=SEED)
    agent = MFEC(env.observation_space, env.action_space, EpsilonGreedy(EPSILON), k=K,
                 capacity=CAPACITY, rng=np.random.default_rng(0))
    return env, agent


def host(trials):
    import mfec_common as mc
    env, agent = make(1)
    agent.feature_table(env)
    F = agent.feature_table(env)
    w = env._tables()
    tab = {'next': w['next'], 'reward': np.asarray(w['rewards'], dtype=np.float64),
           'terminal': np.asarray(w['terminals']).astype(np.uint8),
           'starts': np.asarray(w['starting_states']).astype(np.uint16)}
    t0 = time.perf_counter()
    out, _ = mc.run_restatement(tab, F, [0, trials, STEPS, CAPACITY, K, 0, round(EPSILON * 1e6)], SEED)
    dt = time.perf_counter() - t0
    res = {'host': 'restatement', 'trials': trials, 'steps': len(out['state']),
           'steps_per_s': len(out['state']) / dt}
    src = os.environ.get('COBEL_REFERENCE_SRC')
    if src:
        try:
            sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
            import gen_mfec
            t0 = time.perf_counter()
            d = gen_mfec.case('track', 'onehot', 0, trials, STEPS, 80, K, 0, EPSILON)
            res['reference_steps_per_s'] = len(d['state']) / (time.perf_counter() - t0)
            res['reference_note'] = 'capacity 80 (the recorder keeps the trees to one leaf)'
        except Exception as err:      # noqa: BLE001  (no scikit-learn, no checkout)
            res['reference_error'] = repr(err)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', default='1,1024,16384')
    ap.add_argument('--trials', type=int, default=500)
    ap.add_argument('--warm-trials', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--host-trials', type=int, default=60)
    a = ap.parse_args()
    import torch
    for n in [int(x) for x in a.instances.split(',')]:
        env, agent = make(n)
        agent.train(env, a.warm_trials, STEPS)
        torch.cuda.synchronize()
        sessions = []
        for _ in range(a.repeats):
            before = agent.env_steps()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            agent.train(env, a.trials, STEPS)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            steps = agent.env_steps() - before
            sessions.append({'ms': round(ms, 3), 'steps': steps, 'steps_per_s': steps / (ms * 1e-3)})
        lens = agent._len.float().mean(dim=0).cpu().numpy().round(1).tolist()
        print(json.dumps({'instances': n, 'trials': a.trials, 'sessions': sessions,
                          'mean_buffer_len': lens}), flush=True)
        del env, agent
        torch.cuda.empty_cache()
    print(json.dumps(host(a.host_trials)), flush=True)


if __name__ == '__main__':
    main()
