"""Fuzz of the Rescorla-Wagner kernels: random observation sizes, schedules, policies, learning
rates and step caps; every instance of the device run is compared bit for bit with the restatement
of tests/rw_common.py.

    python scripts/fuzz_rw.py FIRST LAST        # seeds FIRST .. LAST - 1

tests/test_gpu_rw.py runs the slice 0 .. 19.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import rw_common as rc  # noqa: E402


def run_case(seed: int) -> str:
    rng = np.random.default_rng(1000 + seed)
    D = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 48, 64]))
    N = int(rng.choice([1, 2, 3, 7, 16, 17, 40]))
    n_sched = int(rng.integers(1, 4))
    kind = str(rng.choice(['rw', 'rw_overwrite', 'proportional', 'threshold', 'sigmoid']))
    nb_actions = int(rng.integers(1, 4)) if kind.startswith('rw') else 2
    overwrite = kind == 'rw_overwrite'
    n_trials, max_len = int(rng.integers(6, 16)), int(rng.integers(1, 5))
    schedules, obs = rc.random_design(rng, D, n_sched, n_trials, max_len, nb_actions,
                                      arrays=overwrite, dense=bool(rng.random() < 0.7))
    policy, per_instance = None, None
    reverse = bool(rng.random() < 0.5)
    if kind == 'proportional':
        policy = ('proportional', dict(value_max=float(rng.choice([1.0, 1.5])), code_reverse=reverse))
        per_instance = {'value_max': 1.0 + rng.random(N)} if rng.random() < 0.5 else None
    elif kind == 'threshold':
        policy = ('threshold', dict(threshold=0.5, window=float(rng.choice([0.0, 0.2, 0.6])),
                                    value_max=float(D) / 4 + 0.5, code_reverse=reverse))
        per_instance = {'threshold': 0.35 + 0.3 * rng.random(N)} if rng.random() < 0.5 else None
    elif kind == 'sigmoid':
        policy = ('sigmoid', dict(scale=float(rng.choice([1.0, 4.0])), value_max=float(D) / 4 + 0.5,
                                  code_reverse=reverse))
        per_instance = {'threshold': rng.random(N), 'scale': 4 * rng.random(N)} \
            if rng.random() < 0.5 else None
    # (rates that keep the weights bounded on dense observations: the sum of squares grows with D)
    top = 0.5 / max(1.0, D / 3.0)
    lr = [0.6 * top, tuple(top * rng.random(D)), top * rng.random(N), top * rng.random((N, D))][
        int(rng.integers(4))]
    if type(lr) is not float and np.shape(lr) == (N,) and N == D:
        lr = 0.6 * top
    # a session may not run past the last trial: caps below the longest trial hold instances back
    sessions, left = [], n_trials
    for k in range(3):
        t = int(rng.integers(1, max(2, left // 2 + 1)))
        t = min(t, left)
        if t == 0:
            break
        sessions.append(('test' if k == 1 else 'train', t, int(rng.integers(1, max_len + 2))))
        left -= t
    w0 = rng.random((N, D)) / D
    ids = rng.choice(1000, N, replace=False)
    pol_overrides = per_instance
    ag, env = rc.device_run(schedules if n_sched > 1 else schedules[0], obs, nb_actions, overwrite,
                            policy, None, lr, sessions, n_envs=N, instance_ids=ids, w0=w0,
                            pol_overrides=pol_overrides)
    rc.compare_instances(ag, env, schedules, obs, nb_actions, overwrite, policy, lr, sessions, w0,
                         ids, per_instance, what='seed %d' % seed)
    return 'seed %3d: %-12s D %2d N %2d schedules %d trials %2d sessions %s' % (
        seed, kind, D, N, n_sched, n_trials, [(k[0], t, s) for k, t, s in sessions])


def main() -> None:
    first, last = int(sys.argv[1]), int(sys.argv[2])
    for seed in range(first, last):
        print(run_case(seed), flush=True)
    print('fuzz_rw: seeds %d .. %d agree' % (first, last - 1))


if __name__ == '__main__':
    main()
