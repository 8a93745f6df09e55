"""Time of a PMA training session with and without per-instance parameter sets: the demo's
configuration (5 x 5 world of demo_pma.py, masked actions, gamma_q 0.99, batch 32, 50 steps, the
need of timed-out trials on the device) on 16 384 instances.

    python scripts/experiments/pma_sets/time_sets.py [--tree DIR] [--sets K] [--repeats R]

``--tree DIR`` imports the package from another checkout (a build of the parent commit) so that the
same script times both; ``--sets K`` (this tree only) spreads K parameter sets — K values of
``learning_rate_q`` around 0.9 — over the instances, 0 runs the scalar launch.  One process times
one configuration: warm-up sessions, then R sessions of 4 trials, each between two device events
with the device idle before it.  Prints one JSON line; alternate the configurations from the
shell.
"""
import argparse
import json
import os
import sys

import numpy as np


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.dirname(
        os.path.dirname(os.path.abspath(__file__))))))
    ap.add_argument('--sets', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--instances', type=int, default=16384)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, 'cobel-rl_amd'))
    import torch
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.misc.gridworld_tools import make_gridworld
    from cobel_amd.policy import EpsilonGreedy
    n = args.instances
    walls = [(3, 4), (4, 3), (8, 9), (9, 8), (13, 14), (14, 13), (18, 19), (19, 18)]
    w = make_gridworld(5, 5, terminals=[4], rewards=np.array([[4, 10]]), goals=[4],
                       invalid_transitions=walls)
    w['starting_states'] = np.array([12])
    env = Gridworld(w, n_envs=n, seed=20240, device=torch.device('cuda', 0))
    mem = PMAMemory(env.world['sas'], EpsilonGreedy(0.1), gamma_q=0.99)
    mem.offline_need = 'device'
    agent = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    agent.mask_actions = True
    if args.sets:
        mem.learning_rate_q = 0.9 - (np.arange(n) % args.sets) * (0.5 / args.sets)
    times = []
    for k in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        agent.train(env, 4, 50, 32)
        t1.record()
        torch.cuda.synchronize()
        if k >= args.warmup:
            times.append(t0.elapsed_time(t1))
    sets = mem._psets['agent']['n'] if args.sets else 0
    print(json.dumps({'tree': tree, 'sets': sets, 'instances': n, 'ms': [round(t, 3) for t in times],
                      'median_ms': round(float(np.median(times)), 3),
                      'spread_ms': round(float(max(times) - min(times)), 3)}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
