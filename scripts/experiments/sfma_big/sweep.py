"""Throughput of the streaming SFMA form (csrc/sfma_big.hip) by world size, and against the
LDS-resident four-wave form where both run.

    python scripts/experiments/sfma_big/sweep.py [--out profiles/sfma_big_sweep.json] [--only NAME ...]

The driver starts one child process per step, each under its own time limit, and stops at the
first one that does not end with status 0: nothing is started on the GPU after a fault.  A step
times ``SFMA.train`` (Euclidean metric, mode ``default``, B = 32; one warm-up trial, then three
windows of 4 trials each) with HIP events and reads the kernel's own counts of environment steps
and reactivations.  Rates are given for the fastest, the median and the slowest window.

``bytes_per_reactivation`` is the traffic the form asks for by construction, not a counter: three
passes over the 4S strengths (maximum rating; sum and maximum of the weights; locating the draw:
3 x 32 S bytes) and the similarity row of the current state — 8 S once where the plan stages it in
LDS, 8 bytes per experience and pass (3 x 32 S) where it is read in place.  Collect ``rocprofv3 --kernel-trace
--stats`` and any ``--pmc`` pass in runs of their own, with this script after ``--``.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, 'cobel-rl_amd'))

# name: (height, width, force the streaming form, time limit of the step in seconds, threads per
#        instance forced through COBEL_DEBUG_SFMA_STREAM_THREADS or 0)
STEPS = {
    'lds_23x23': (23, 23, False, 120, 0), 'stream_23x23': (23, 23, True, 120, 0),
    'lds_35x36': (35, 36, False, 120, 0), 'stream_35x36': (35, 36, True, 120, 0),
    'stream_36x36': (36, 36, False, 120, 0), 'stream_48x48': (48, 48, False, 120, 0),
    'stream_64x64': (64, 64, False, 180, 0), 'stream_90x90': (90, 90, False, 240, 0),
    'stream_127x127': (127, 127, False, 420, 0),
    'stream512_36x36': (36, 36, False, 120, 512), 'stream512_64x64': (64, 64, False, 180, 512),
    'stream512_90x90': (90, 90, False, 240, 512),
}


def step(name: str) -> dict:
    if STEPS[name][4]:
        os.environ['COBEL_DEBUG'] = '1'
        os.environ['COBEL_DEBUG_SFMA_STREAM_THREADS'] = str(STEPS[name][4])
    import numpy as np
    import torch
    from cobel_amd import _lib
    from cobel_amd.agent import SFMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import SFMAMemory
    from cobel_amd.memory.utils import Euclidean
    from cobel_amd.misc.gridworld_tools import make_gridworld
    from cobel_amd.policy import EpsilonGreedy
    import ctypes as C
    h, w, force, _, forced_threads = STEPS[name]
    S = h * w
    plan = (C.c_int32 * 4)()
    _lib.check(_lib.lib().cobel_sfma_plan(S, _lib.F_SFMA_STREAM if force else 0, C.byref(plan)))
    form, lds, threads, _ = list(plan)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # workgroups one CU holds: by LDS (160 KiB) and by its 2 048 threads; the chip is filled once
    per_cu = max(1, min(160 * 1024 // lds, 2048 // threads))
    n = min(65536, cus * per_cu)
    goal = w - 1
    world = make_gridworld(h, w, terminals=[goal], rewards=np.array([[goal, 1.0]]), goals=[goal])
    env = Gridworld(world, n_envs=n, seed=7)
    mem = SFMAMemory(Euclidean(w, h).D, S, 4)
    agent = SFMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    agent.force_stream_kernel = force
    steps, B = 2 * max(h, w), 32
    agent.train(env, 1, steps, B)                     # warm-up: tables bound, metric uploaded
    torch.cuda.synchronize()
    wins = []
    for _ in range(3):
        s0, r0 = agent.env_steps(), int(agent.replays_done)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        agent.train(env, 4, steps, B)
        t1.record()
        torch.cuda.synchronize()
        sec = t0.elapsed_time(t1) * 1e-3
        wins.append((sec, agent.env_steps() - s0, int(agent.replays_done) - r0))
    react = sorted(r / t for t, _, r in wins)
    esteps = sorted(e / t for t, e, _ in wins)
    rows_in_lds = (lds - 1024) // S >= 24
    return dict(name=name, states=S, form=form, lds_bytes=lds, threads=threads, instances=n,
                window_seconds=[t for t, _, _ in wins],
                reactivations_per_window=[r for _, _, r in wins],
                reactivations_per_s=dict(min=react[0], median=react[1], max=react[2]),
                env_steps_per_s=dict(min=esteps[0], median=esteps[1], max=esteps[2]),
                bytes_per_reactivation=(3 * 32 * S + (8 * S if rows_in_lds else 3 * 32 * S))
                if form else 0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument('--step')
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sfma_big_sweep.json'))
    a = ap.parse_args()
    if a.step:
        print('RESULT ' + json.dumps(step(a.step)), flush=True)
        return 0
    rows = []
    for name in (a.only or STEPS):
        t = time.time()
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name],
                               timeout=STEPS[name][3], capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print('%s: time limit; stopping' % name, flush=True)
            break
        got = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
        if p.returncode != 0 or not got:
            print('%s: status %d; stopping\n%s' % (name, p.returncode, p.stderr[-2000:]), flush=True)
            break
        rows.append(json.loads(got[-1][7:]))
        print('%s: %.1f s  %s' % (name, time.time() - t, got[-1][7:]), flush=True)
    with open(a.out, 'w') as f:
        json.dump(dict(rows=rows), f, indent=1)
    return 0 if len(rows) == len(a.only or STEPS) else 1


if __name__ == '__main__':
    sys.exit(main())
