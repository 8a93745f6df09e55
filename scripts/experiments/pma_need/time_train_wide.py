"""PMA.train on a wide memory with ``offline_need = 'host'`` against ``'device'`` (docs/MEASUREMENTS.md
§27), by the method of time_train.py.

Worlds seeded_world(16, 20, 8) (320 states) and seeded_world(32, 32, 9) (1 024 states), N in {8, 64},
trials of 20 steps, batch 8, ``need_workspace = N``, both modes in one process.  Per configuration:
wall time per trial (the session timed between two ``torch.cuda.synchronize()``, after one warm-up
session on a memory of its own), the share of trials that timed out, and the time of
``_need_device`` alone from events — the fills of ``need`` and ``status`` and the launches of
``cobel_pma_stationary_wide`` — median of 20, on the tables the session left, selecting all
instances and selecting by the session's ``last``.  Then, at 128 states (seeded_world(8, 16, 3)
after a session), the same event time of the LDS kernel and of the wide kernels on the same tables.

    python scripts/experiments/pma_need/time_train_wide.py [--trials 3] [--steps 20] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import pma_common as pc  # noqa: E402

WORLDS = {'seeded_16x20': lambda: pc.seeded_world(16, 20, 8),
          'seeded_32x32': lambda: pc.seeded_world(32, 32, 9)}


def make(world, n, mode, wide=True):
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    env = Gridworld(world, n_envs=n, seed=2024)
    kw = {'wide': True, 'need_workspace': n} if wide else {}
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, **kw)
    mem.offline_need = mode
    return env, PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem), mem


def kernel_us(mem, select, reps=20):
    mem._need_device(select)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        mem._need_device(select)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def lds_against_wide(args) -> list:
    """128 states: the LDS kernel and the wide kernels on the tables one session left."""
    world = pc.seeded_world(8, 16, 3)
    rows = []
    for n in (8, 64):
        env, ag, narrow = make(world, n, 'device', wide=False)
        ag.train(env, 4, args.steps, batch_size=args.batch)
        torch.cuda.synchronize()
        _, _, wide = make(world, n, 'device')
        wide.bind(n)
        wide._dev['T'].copy_(narrow._dev['T'])
        same = torch.equal(narrow._need_device(None), wide._need_device(None))
        rows.append({'states': 128, 'n': n, 'lds_us': kernel_us(narrow, None),
                     'wide_us': kernel_us(wide, None), 'same_bits': bool(same)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--trials', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--modes', default='device,host', help="'device' alone skips the host column")
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for wname, build in WORLDS.items():
        world = build()
        for n in (8, 64):
            row = {'world': wname, 'states': int(world['states']), 'n': n}
            for mode in args.modes.split(','):
                env, ag, mem = make(world, n, mode)
                ag.train(env, 1, args.steps, batch_size=args.batch)       # warm-up
                torch.cuda.synchronize()
                env, ag, mem = make(world, n, mode)
                t0 = time.perf_counter()
                ag.train(env, args.trials, args.steps, batch_size=args.batch)
                torch.cuda.synchronize()
                row[mode + '_ms_per_trial'] = (time.perf_counter() - t0) * 1e3 / args.trials
                row[mode + '_timed_out_last_trial'] = float((ag._last < 0).float().mean().item())
                if mode == 'device':
                    row['kernel_all_us'] = kernel_us(mem, None)
                    row['kernel_last_us'] = kernel_us(mem, ag._last)
                    row['degenerate'] = int(mem.need_status.sum().item())
                print(json.dumps({k: row[k] for k in row}), flush=True)
            rows.append(row)
    print('| world | S | N | host ms / trial | device ms / trial | ratio | kernels, all N (us) | '
          'kernels, select = last (us) | timed out (last trial) |')
    print('|---|---|---|---|---|---|---|---|---|')
    for r in rows:
        r.setdefault('host_ms_per_trial', float('nan'))
        print('| %s | %d | %d | %.1f | %.2f | %.0f | %.0f | %.0f | %.0f %% |' % (
            r['world'], r['states'], r['n'], r['host_ms_per_trial'], r['device_ms_per_trial'],
            r['host_ms_per_trial'] / r['device_ms_per_trial'], r['kernel_all_us'],
            r['kernel_last_us'], 100 * r['device_timed_out_last_trial']))
    small = lds_against_wide(args)
    print('| S | N | LDS kernel (us) | wide kernels (us) | same bits |')
    print('|---|---|---|---|---|')
    for r in small:
        print('| %d | %d | %.0f | %.0f | %s |' % (r['states'], r['n'], r['lds_us'], r['wide_us'],
                                                 r['same_bits']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'train': rows, 'states_128': small}, f, indent=1)


if __name__ == '__main__':
    main()
