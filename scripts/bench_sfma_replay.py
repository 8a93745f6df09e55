#!/usr/bin/env python3
"""SFMAMemory.replay_batch on one MI355X: replays/s and reactivations/s of K = 64 replays of length
L = 32 from the frozen memories of 1 024 instances trained for 20 trials — on the 5 x 5 world of
demo/gridworld/demo_sfma.py's size (LDS-resident form, one wavefront per replay) and on a 32 x 32
open field in the streaming form (a world name with an `s` behind it asks for that form; without
it 1 024 states take the four-wave LDS form).

Method (docs/MEASUREMENTS.md): one process, the GPU warmed by the training itself and two untimed
calls; then `--windows` windows of `--calls` calls each between two HIP events on the stream the
calls run on, no host synchronisation inside a window; reactivations counted from the lengths the
calls return (copied after the window); median window, slowest and fastest next to it.  Two
comparison figures: the NumPy restatement (oracle/sfma_loop.py) doing the same replays on one host
core, and the reactivation rate inside SFMA.train on the same world and instance count (replays_done
of the fused kernel over a timed window of trials).

    python scripts/bench_sfma_replay.py [--instances 1024] [--k 64] [--length 32] [--worlds 5x5,32x32s]

Prints one JSON line per world."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 2024


def build(h, w, n, stream):
    from cobel_amd.agent import SFMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import SFMAMemory
    from cobel_amd.memory.utils import Euclidean
    from cobel_amd.misc.gridworld_tools import make_open_field
    from cobel_amd.policy import EpsilonGreedy
    world = make_open_field(h, w, 0, 1)
    env = Gridworld(world, n_envs=n, seed=SEED)
    D = Euclidean(w, h).D
    agent = SFMA(env.observation_space, env.action_space, EpsilonGreedy(0.1),
                 SFMAMemory(D, h * w, 4))
    agent.force_stream_kernel = stream
    return world, env, agent, D


def timed(torch, fn, windows):
    """Milliseconds of `windows` runs of fn() between two events each, and what fn returned."""
    ms, out = [], []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        out.append(r)
    return np.array(ms), out


def rate(count, ms):
    r = np.sort(np.asarray(count, dtype=np.float64) / (ms * 1e-3))
    return {'median': float(np.median(r)), 'slowest': float(r[0]), 'fastest': float(r[-1])}


def one_world(h, w, stream, args):
    import torch
    from cobel_amd import _lib
    from oracle import sfma_loop
    from oracle.philox import STREAM_MEMORY, TapeRNG
    n, K, L = args.instances, args.k, args.length
    steps = 2 * max(h, w)
    world, env, agent, D = build(h, w, n, stream)
    M = agent.M
    agent.train(env, 20, steps, 32)
    torch.cuda.synchronize()
    M.launch_flags = _lib.F_SFMA_STREAM if stream else 0
    # the in-train rate: four more trials between events, reactivations from the kernel's counter
    before = int(agent.replays_done.item())
    ms_train, _ = timed(torch, lambda: agent.train(env, 4, steps, 32), 1)
    in_train = (int(agent.replays_done.item()) - before) / (ms_train[0] * 1e-3)

    # the device calls as replay_batch makes them, without the host-side decoding of the events
    m, dev = M._mem(_lib.SFM_STRIDED)
    events = torch.zeros((n, K, L * _lib.SFMA_EVENT_BYTES), dtype=torch.uint8, device=dev)
    lengths = torch.zeros((args.calls, n, K), dtype=torch.int32, device=dev)
    st = _lib.current_stream(dev)
    import ctypes as C

    def window():
        for c in range(args.calls):
            _lib.check(_lib.lib().cobel_sfma_replay(C.byref(m), K, L, None, None, _lib.ptr(events),
                                                    _lib.ptr(lengths[c]), None, st))
        return None
    window()
    window()
    torch.cuda.synchronize()
    counts = []
    ms = []
    for _ in range(args.windows):
        t, _ = timed(torch, window, 1)
        ms.append(t[0])
        counts.append(int(lengths.sum().item()))
    ms = np.array(ms)
    # the same replays by the restatement on one host core (instance 0, a few of them)
    ref = sfma_loop.RefSFMAMemory(D, h * w, 4, TapeRNG(SEED, 0, STREAM_MEMORY, double_sub=1),
                                  dtype=np.float32)
    ref.C = np.array(M.C[0])
    ref.rewards, ref.states, ref.terminals = M.rewards[0], M.states[0], M.terminals[0]
    t0, done, reps = time.perf_counter(), 0, 0
    while time.perf_counter() - t0 < args.oracle_seconds:
        done += len(ref.replay(L))
        reps += 1
    dt = time.perf_counter() - t0
    plan = M.launch_plan()
    return {
        'world': '%dx%d' % (h, w), 'states': h * w, 'instances': n, 'K': K, 'L': L,
        'form': plan[0], 'lds_bytes': plan[1], 'threads': plan[2],
        'calls_per_window': args.calls, 'window_ms': [float(x) for x in ms],
        'replays_per_s': rate([n * K * args.calls] * len(ms), ms),
        'reactivations_per_s': rate(counts, ms),
        'mean_length': counts[0] / (n * K * args.calls),
        'oracle_one_core': {'replays_per_s': reps / dt, 'reactivations_per_s': done / dt},
        'in_train_reactivations_per_s': in_train, 'in_train_window_ms': float(ms_train[0]),
    }


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--instances', type=int, default=1024)
    ap.add_argument('--k', type=int, default=64)
    ap.add_argument('--length', type=int, default=32)
    ap.add_argument('--calls', type=int, default=4)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--oracle-seconds', type=float, default=2.0)
    ap.add_argument('--worlds', default='5x5,32x32s')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'
    for name in args.worlds.split(','):
        h, w = [int(x) for x in name.rstrip('s').split('x')]
        print(json.dumps(one_world(h, w, name.endswith('s'), args)), flush=True)


if __name__ == '__main__':
    main()
