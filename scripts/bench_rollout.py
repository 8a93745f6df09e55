#!/usr/bin/env python3
"""`agent.rollout` on one MI355X against its two yardsticks: `agent.test` of the same session, and
the only other route to the same data — launches of one environment step (`step_budget = 1`) with
`last_exp` copied out after each.

Shapes (`--shape`): `c2` — 65 536 instances on the 5x5 open field, 50 steps, 20 trials; `c3` —
65 536 instances over 64 obstacle mazes of 32x32, 200 steps, 10 trials.  Dyna-Q, epsilon 0.1, a
policy_test of its own, tables pre-trained for `--pretrain` trials so that trials end where a
trained agent's do.

Method (docs/MEASUREMENTS.md section 1): one process; three agents and environments built alike —
they run the same sessions draw for draw — one for `test()`, one for `rollout()` with grouped
stores, one with a store per record entry (`rollout_element_stores`).  One untimed session each,
then `--repeats` rounds in which the three run the next session one after the other, each between
two HIP events on its stream (the record's allocation and the two fills of its padding are inside
the window of a rollout: they are part of the call).  A plain device write of the record's bytes
(`Tensor.fill_` on a buffer of that size) is timed in the same rounds.  The per-step route is
timed over `--step-launches` launches and scaled to the launches the session would need (steps x
trials: every instance runs until the slowest has finished).  Record bytes: the padded record the
call produces, N x trials x (3 x steps + 6); `entry_bytes` counts only what the kernel itself
stores (3 bytes per executed step, 6 per trial).

    python scripts/bench_rollout.py [--shape c2,c3] [--repeats 5]

Prints one JSON line per shape."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 2024
SHAPES = {'c2': dict(n=65536, steps=50, trials=20, batch=8),
          'c3': dict(n=65536, steps=200, trials=10, batch=8)}


def make(shape: str, n: int, pretrain: int):
    from cobel_amd.agent import DynaQ
    from cobel_amd.interface import Gridworld
    from cobel_amd.misc.gridworld_tools import make_obstacle_maze, make_open_field
    from cobel_amd.policy import EpsilonGreedy
    cfg = SHAPES[shape]
    worlds = [make_open_field(5, 5, 0, 1)] if shape == 'c2' else \
        [make_obstacle_maze(32, 32, 1234 + k) for k in range(64)]
    env = Gridworld(worlds, n_envs=n, seed=SEED)
    env.live_world = False
    agent = DynaQ(env.observation_space, env.action_space, EpsilonGreedy(0.1), EpsilonGreedy(0.1))
    agent.track_instances = True
    if pretrain:
        agent.train(env, pretrain, cfg['steps'], cfg['batch'])
    return env, agent


def timed(torch, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def per_step_route(torch, env, agent, steps: int, launches: int) -> float:
    """Milliseconds per launch of one environment step with `last_exp` copied out."""
    from cobel_amd import _lib
    pol, flags, first = agent._session_begin(env, 1, False)
    keep = torch.empty((launches,) + tuple(agent._last_exp.shape), dtype=torch.int32,
                       device=agent.device)

    def run():
        for k in range(launches):
            agent._launch(env, pol, flags, first + 1000000, steps, 1, 0)
            keep[k].copy_(agent._last_exp)
    run()
    ms, _ = timed(torch, run)
    agent.inst[:, _lib.I_TRIAL] = first       # (the probe is not a session: trial counters back)
    agent.inst[:, _lib.I_FLAGS] = 0
    agent._session_end(pol, env)
    return ms / launches


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def run_shape(shape: str, a) -> dict:
    import torch
    from cobel_amd.monitor.trajectory import record_bytes
    cfg = SHAPES[shape]
    n, steps, trials = a.instances or cfg['n'], cfg['steps'], cfg['trials']
    rigs = {k: make(shape, n, a.pretrain) for k in ('test', 'rollout', 'rollout_element')}
    rigs['rollout_element'][1].rollout_element_stores = True
    nbytes = record_bytes(n, trials, steps)
    plain = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    ms = {k: [] for k in list(rigs) + ['plain_write']}
    entry_bytes = lengths = None
    for r in range(a.repeats + 1):
        row = {}
        for k, (env, agent) in rigs.items():
            if k == 'test':
                row[k], _ = timed(torch, lambda: agent.test(env, trials, steps))
            else:
                row[k], rec = timed(torch, lambda: agent.rollout(env, trials, steps))
                executed = int(rec.length.sum().item())
                entry_bytes, lengths = 3 * executed + 6 * n * trials, executed / (n * trials)
                del rec
        row['plain_write'], _ = timed(torch, lambda: plain.fill_(255))
        if r:      # (round 0 is the warm-up)
            for k, v in row.items():
                ms[k].append(v)
    med = {k: median(v) for k, v in ms.items()}
    step_ms = per_step_route(torch, *rigs['test'], steps, a.step_launches)
    extra = med['rollout'] - med['test']
    return {
        'shape': shape, 'instances': n, 'steps': steps, 'trials': trials,
        'plan': rigs['rollout'][1].rollout_plan, 'record_bytes': nbytes,
        'entry_bytes': entry_bytes, 'mean_trial_length': round(lengths, 2),
        'ms_median': {k: round(v, 3) for k, v in med.items()},
        'ms_all': {k: [round(x, 3) for x in v] for k, v in ms.items()},
        'rollout_over_test': round(med['rollout'] / med['test'], 3),
        'rollout_minus_test_ms': round(extra, 3),
        'record_GBps_over_rollout': round(nbytes / med['rollout'] * 1e-6, 1),
        'record_GBps_over_extra': round(nbytes / extra * 1e-6, 1) if extra > 0 else None,
        'plain_write_GBps': round(nbytes / med['plain_write'] * 1e-6, 1),
        'per_step_route': {'ms_per_launch': round(step_ms, 4), 'launches': steps * trials,
                           'ms_session': round(step_ms * steps * trials, 1)},
    }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='c2,c3')
    ap.add_argument('--instances', type=int, default=0, help='override the instance count')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--pretrain', type=int, default=20)
    ap.add_argument('--step-launches', type=int, default=200)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_rollout.py needs a GPU'
    for shape in a.shape.split(','):
        print(json.dumps(run_shape(shape, a)), flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
