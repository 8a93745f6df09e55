#!/usr/bin/env python3
"""Planning updates per second of DynaQ.replay(50, 512) on C3's worlds (65 536 instances over 64
32 x 32 obstacle mazes) with trained agents, in both forms of k_tab_replay, next to the planning
updates per second the fused C3 launch achieves in the same process (batches_done x 50 / launch
time).  Not part of bench.py.

Method (docs/MEASUREMENTS.md): one process; the agents are trained by `--pretrain` untimed fused
launches of 512 steps, which also warm the GPU; every timed shape is run once untimed first; then
`--windows` windows per leg between two HIP events on the stream the calls run on, the three legs
(wave form, lane form, fused launch) alternating, no host synchronisation inside a window; median
window, slowest and fastest next to it.  Replaying changes Q, so later windows plan on tables that
have been planned on more: the spread shows what that does.  The wave and lane forms are checked
to leave the same bits on the way (one call each from the same state).

    python scripts/experiments/dynaq_replay_rate.py [--instances 65536] [--batch 50]
        [--n-batches 512] [--pretrain 12] [--windows 5]

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def spread(rates):
    r = np.sort(np.asarray(rates, dtype=np.float64))
    return {'median': float(np.median(r)), 'slowest': float(r[0]), 'fastest': float(r[-1])}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=65536)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--n-batches', type=int, default=512)
    ap.add_argument('--pretrain', type=int, default=12)
    ap.add_argument('--windows', type=int, default=5)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU: there is no fallback'
    import bench
    from cobel_amd import _lib
    dev = torch.device('cuda', 0)
    n, B, K = args.instances, args.batch, args.n_batches
    cfg = dict(bench.CONFIGS['C3'], instances=n, batch=B)
    env, agent = bench.build_agent('C3', cfg, n, 0, dev)
    runner = bench.Runner(cfg, env, agent)
    for _ in range(args.pretrain):
        runner.launch()
    torch.cuda.synchronize()
    trained = float((agent._q.abs().amax(dim=(1, 2)) > 0).float().mean())

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    def replay(lane):
        agent.extra_flags = _lib.F_REPLAY_LANE if lane else 0
        try:
            agent.replay(B, K)
        finally:
            agent.extra_flags = 0

    def fused():
        before = int(agent.batches_done.item())
        s = window(runner.launch)
        return (int(agent.batches_done.item()) - before) * B / s

    # the two forms leave the same bits (and every timed shape has run once)
    q0, c0 = agent._q.clone(), agent.M.counter.clone()
    replay(False)
    q_wave = agent._q.clone()
    agent._q.copy_(q0)
    agent.M.counter.copy_(c0)
    replay(True)
    assert torch.equal(agent._q, q_wave), 'wave and lane form differ'
    agent._q.copy_(q0)
    agent.M.counter.copy_(c0)
    runner.launch()
    torch.cuda.synchronize()

    plans = {}
    for lane in (False, True):
        agent.extra_flags = _lib.F_REPLAY_LANE if lane else 0
        plans['lane' if lane else 'wave'] = agent.replay_plan(B, K)
    agent.extra_flags = 0
    rates = {'wave': [], 'lane': [], 'fused': []}
    for _ in range(args.windows):
        rates['wave'].append(n * K * B / window(lambda: replay(False)))
        rates['lane'].append(n * K * B / window(lambda: replay(True)))
        rates['fused'].append(fused())
    out = {
        'what': 'planning updates per second, DynaQ.replay(%d, %d) on C3 worlds, %d instances'
                % (B, K, n),
        'device': torch.cuda.get_device_name(0),
        'instances_with_nonzero_q': trained, 'pretrain_launches': args.pretrain,
        'plan': plans, 'fused_kernel': runner.describe(),
        'replay_wave': spread(rates['wave']), 'replay_lane': spread(rates['lane']),
        'fused_c3_launch_planning': spread(rates['fused']),
        'windows': args.windows,
    }
    out['wave_over_fused'] = out['replay_wave']['median'] / out['fused_c3_launch_planning']['median']
    out['lane_over_fused'] = out['replay_lane']['median'] / out['fused_c3_launch_planning']['median']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
