"""The SFMA metrics on the device against the host path (docs/MEASUREMENTS.md §28).

One case per process, so that a job script gives each device step a time limit of its own:

    python scripts/experiments/metric/time_metric.py sr 1024 [--worlds 64] [--no-host]
    python scripts/experiments/metric/time_metric.py dr 4096 --rank 32

``sr S``   ``SR(next, 0.9, compute='device')`` on the open field of S states with two walls (S a
           product width x height from SHAPES), W worlds in one call: the time of
           ``update_transitions()`` — table upload, init and elimination — from events, median of
           ``--reps`` after one warm-up call.
``dr S``   ``DR(..., compute='device').update_transitions()`` — the Woodbury step alone, D0 kept — on
           a world whose invalid transitions start from ``--rank`` states.
Host column: what the parent commit ran for the same matrix on this machine's CPUs —
``SR(next, 0.9)`` per world (``np.linalg.inv``) or ``DR.update_transitions()`` (the host Woodbury
products) — plus the upload of the float64 stack, between two ``perf_counter`` readings with a
``torch.cuda.synchronize()`` before the second.  Prints one JSON line."""
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

import metric_common as mc  # noqa: E402

SHAPES = {1024: (32, 32), 4096: (64, 64), 16383: (127, 129)}


def event_ms(call, reps):
    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main() -> None:
    from cobel_amd.memory.utils import DR, SR
    ap = argparse.ArgumentParser()
    ap.add_argument('kind', choices=('sr', 'dr'))
    ap.add_argument('states', type=int, choices=sorted(SHAPES))
    ap.add_argument('--worlds', type=int, default=1)
    ap.add_argument('--rank', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    w, h = SHAPES[args.states]
    S, W, dev = w * h, args.worlds, torch.device('cuda', 0)
    row = {'kind': args.kind, 'states': S, 'worlds': W}
    if args.kind == 'sr':
        tabs = [mc.with_walls(w, h, [(w + 1, w + 2), (3 * w + 5 + i, 4 * w + 5 + i)])[0]
                for i in range(W)]
        m = SR(tabs if W > 1 else tabs[0], 0.9, compute='device', device=dev)
        row['device_ms'] = event_ms(m.update_transitions, args.reps)
        if not args.no_host:
            t0 = time.perf_counter()
            D = np.stack([SR(t, 0.9).D for t in tabs])
            t1 = time.perf_counter()
            up = torch.as_tensor(D, device=dev)
            torch.cuda.synchronize()
            row['host_ms'], row['upload_ms'] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
            row['max_abs_diff'] = float((up - m._D).abs().max().item())
    else:
        nxt, inv = mc.world_of_rank(w, h, args.rank, seed=args.rank)
        row['rank'] = args.rank
        m = DR(w, h, nxt, 0.9, inv, compute='device', device=dev)
        row['device_ms'] = event_ms(m.update_transitions, args.reps)
        if not args.no_host:
            host = DR(w, h, nxt, 0.9, inv)
            t0 = time.perf_counter()
            host.update_transitions()
            t1 = time.perf_counter()
            up = torch.as_tensor(host.D, device=dev)
            torch.cuda.synchronize()
            row['host_ms'], row['upload_ms'] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
            row['max_abs_diff'] = float((up - m.D).abs().max().item())
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
