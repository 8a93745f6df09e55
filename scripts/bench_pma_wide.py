#!/usr/bin/env python3
"""PMA's wide form on one MI355X: replay rounds/s of `PMAMemory.replay(L)` and milliseconds of
`update_sr` (the blocked kernels on the SR in device memory) at S = 132, 272 and 1 024, for one
instance and for `--fill` instances (enough workgroups for every CU), the host's `numpy.linalg.inv`
of the same matrix beside it as context; and what the narrow worlds (S = 25 and 128) would pay for
running through the wide instantiation and the blocked update_sr instead of their own kernels.

Method (docs/MEASUREMENTS.md, as scripts/bench_pma_replay.py): one process, one untimed call first,
`--windows` windows of `--calls` device calls each between two HIP events on the calls' stream, no
host synchronisation inside a window; median window, fastest and slowest beside it.  Memories are
filled by a seeded walk of stores; the replay starts at the world's start state with the host's
initial SR.

    python scripts/bench_pma_wide.py [--fill 256] [--windows 7] [--calls 4]

Prints one JSON line per (world, instances)."""
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


def windows_of(torch, fn, windows, calls):
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def memory_of(world, n, wide):
    import pma_common as pc
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    tabs, _ = pc.tables_of(world)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, wide=wide)
    mem.bind(n, seed=SEED)
    for s, a, r, ns, t in pc.walk_stores(tabs, 40, seed=3):
        mem.store({'state': s, 'action': a, 'reward': r, 'next_state': ns, 'terminal': t})
    return mem


def measure(torch, world, n, wide, L, a, blocked=None):
    """blocked: None — the library's own choice; True — COBEL_DEBUG_PMA_SR=blocked."""
    mem = memory_of(world, n, wide)
    S, A = mem.nb_states, mem.nb_actions
    start = np.full(n, int(world['starting_states'][0]), dtype=np.int32)
    q = torch.zeros((n, S, A), dtype=torch.float64, device=mem.device)
    rep_fn = lambda: mem._replay_device(q, None, L, start, None, None)      # noqa: E731
    rep_fn()
    rep = windows_of(torch, rep_fn, a.windows, a.calls)
    if blocked:
        os.environ['COBEL_DEBUG'], os.environ['COBEL_DEBUG_PMA_SR'] = '1', 'blocked'
    try:
        mem.update_sr()
        sr = windows_of(torch, mem.update_sr, a.windows, a.calls)
    finally:
        if blocked:
            del os.environ['COBEL_DEBUG_PMA_SR'], os.environ['COBEL_DEBUG']
    return {'states': S, 'instances': n, 'wide': wide, 'sr_blocked': bool(blocked or S > 128),
            'replay_length': L, 'plan': mem.launch_plan(L), 'replay_ms': rep,
            'replay_rounds_per_s': round(n * L / (rep[0] * 1e-3), 1), 'update_sr_ms': sr}


def host_inv_ms(world, repeats=5):
    import pma_common as pc
    _, sas = pc.tables_of(world)
    M = np.eye(sas.shape[0]) - 0.9 * (sas.sum(axis=1) / sas.shape[1])
    np.linalg.inv(M)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        np.linalg.inv(M)
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--fill', type=int, default=256)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--calls', type=int, default=4)
    a = ap.parse_args()
    import torch
    import pma_common as pc
    import pma_wide_common as pw
    for name, world, L in (('12x11', pw.world_132(), 32), ('17x16', pw.world_272(), 32),
                           ('32x32', pw.world_1024(), 8)):
        host = host_inv_ms(world)
        for n in (1, a.fill):
            out = measure(torch, world, n, True, L, a)
            out.update({'world': name, 'host_inv_ms': host})
            print(json.dumps(out), flush=True)
    # the narrow worlds through their own kernels and through the wide form
    for name, world in (('5x5', pc.demo_world()), ('8x16', pc.seeded_world(8, 16, seed=8))):
        for n in (1, 16384):
            for wide in (False, True):
                out = measure(torch, world, n, wide, 32, a, blocked=wide)
                out['world'] = name
                print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
