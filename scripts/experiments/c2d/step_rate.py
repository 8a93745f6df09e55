"""Environment steps per second of ``cobel_c2d_step`` alone, on the demo's open field (75 edges).

For both robot types: 65 536 instances at every lane mapping the planner allows there, smaller
counts at every mapping (the planner's crossover rests on these), and 64 instances at each
mapping; next to them the rate of the NumPy restatement (tests/c2d_common.py) on one host core.

Timing: device events around a window of back-to-back launches on one stream, after a warm-up of
the same shape; the window is grown until it lasts at least 0.3 s; the median of five windows is
reported with their spread.  Actions are seeded and change every launch, states evolve (robots run
into walls and reach the reward as they do in training).  The rate at 64 instances is that of the
launch, not of the arithmetic.

    python scripts/experiments/c2d/step_rate.py [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

LANES = (1, 4, 16, 64)
COUNTS = (64, 1024, 4096, 16384, 65536)


def demo_arena():
    from cobel_amd.misc import continuous_tools as ct
    room = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    obstacles = [ct.make_rectangle(np.ones(2) / 2, 0.1, 0.1, 45), ct.make_circle(np.array([0.9, 0.1]), 0.05),
                 ct.make_triangle(np.array([0.1, 0.9]), 0.1, 0.1)]
    return room, None, obstacles, np.array([[0.75, 0.75, 10.0]])


def device_rate(torch, robot: str, n: int, lanes: int, seed: int = 7) -> dict:
    from cobel_amd import _lib
    from cobel_amd.interface import Continuous2D
    env = Continuous2D(robot, *demo_arena(), n_envs=n, seed=seed)
    env.lanes_per_instance = lanes
    n_act = int(env.action_space.n)
    gen = torch.Generator(device='cuda').manual_seed(seed)
    actions = torch.randint(0, n_act, (64, n), dtype=torch.uint8, device='cuda', generator=gen)
    c, lib, stream = env.descriptor(), _lib.lib(), _lib.current_stream(env.device)
    args = (_lib.ptr(env._reward), _lib.ptr(env._done), _lib.ptr(env._wall), stream)

    def window(launches: int) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for k in range(launches):
            _lib.check(lib.cobel_c2d_step(C.byref(c), actions[k & 63].data_ptr(), *args))
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    launches = 64
    window(launches)                                    # warm-up: code object, this shape
    while window(launches) < 0.3 and launches < (1 << 20):
        launches *= 2
    rates = sorted(n * launches / window(launches) for _ in range(5))
    return dict(robot=robot, n=n, lanes=lanes, launches=launches, steps_per_s=rates[2],
                lowest=rates[0], highest=rates[-1], us_per_launch=1e6 * n / rates[2],
                wall_share=float(env._wall.float().mean()))


def host_rate(robot: int, steps: int = 3000) -> float:
    import c2d_common as cc
    T, R = cc.geometries()['open_field']
    rng = np.random.default_rng(1)
    box = cc.bounds(T)
    state, _, _, _ = cc.reset(T, T, box, (0.3, 0.3), robot, 7, 0, 0)
    actions = rng.integers(0, 4 if robot == cc.STEP else 3, steps)
    t0 = time.perf_counter()
    for a in actions:
        state, _, _, _ = cc.step(T, R[:1], robot, state, int(a))
    return steps / (time.perf_counter() - t0)


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=None)
    opts = parser.parse_args()
    import torch
    assert torch.cuda.is_available(), 'the step rate is a measurement on the GPU'
    from cobel_amd import _lib
    rows = []
    for robot in ('step', 'wheel'):
        for n in COUNTS:
            plan = (C.c_int32 * 4)()
            _lib.check(_lib.lib().cobel_c2d_plan(n, 75, C.byref(plan)))
            for lanes in LANES:
                row = device_rate(torch, robot, n, lanes)
                row['planner'] = plan[0] == lanes
                row['within_lane_cap'] = n * lanes <= 65536
                rows.append(row)
                print(json.dumps(row), flush=True)
    host = {'step': host_rate(0), 'wheel': host_rate(1)}
    print(json.dumps({'numpy_restatement_steps_per_s': host}), flush=True)
    if opts.out:
        with open(opts.out, 'w') as f:
            json.dump({'device': rows, 'numpy_restatement_steps_per_s': host,
                       'gpu': torch.cuda.get_device_name(0)}, f, indent=1)


if __name__ == '__main__':
    main()
