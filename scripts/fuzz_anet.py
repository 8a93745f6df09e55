#!/usr/bin/env python3
"""Randomised parity sweep for the AssociativeNetwork agent (csrc/anet.hip) against the restatement
of tests/anet_common.py: random observation sizes D (group size G = D rounded up to a power of two,
64 / G instances per wavefront), one to eight outputs, instance counts that leave the last wavefront
partly filled, one to three schedules of different trial lengths so that the instances of a wavefront
drift apart, one-hot or dense observations, noise on or off, both update rules, saturation / rate /
epsilon as scalars, tables or per instance, random instance numbers, and sessions that mix train,
test, rescale, alpha and predict with step caps below the longest trial.  Every instance of the run
is compared with its restatement on ``anet_common.EXACT`` with np.array_equal.

    python scripts/fuzz_anet.py [first_seed] [count]

tests/test_gpu_fuzz_agents.py runs a fixed slice.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

DIMS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 48, 63, 64)
COUNTS = (1, 2, 3, 7, 16, 17, 40, 65)
# The restatement is plain Python: a step costs about 6 G NA operations (two tree sums per output).
# G x NA x N x (steps of one instance) is kept below this, about half a second of host time.
WORK = 400_000
KEYS = ('excitatory', 'inhibitory')


def group_size(D: int) -> int:
    G = 1
    while G < D:
        G *= 2
    return G


def draw_case(seed: int) -> dict:
    import rw_common as rc
    r = np.random.default_rng(seed)
    D, N = int(r.choice(DIMS)), int(r.choice(COUNTS))
    n_actions = int(r.integers(2, 10))
    NA, G = n_actions - 1, group_size(D)
    n_sched = int(r.integers(1, 4))
    n_trials, max_len = int(r.integers(6, 16)), int(r.integers(1, 5))
    cap = max(3, WORK // (G * NA * N))
    while n_trials * max_len > cap and (n_trials > 3 or max_len > 1):
        if max_len > 1 and (n_trials <= 3 or r.random() < 0.5):
            max_len -= 1
        else:
            n_trials -= 1
    overwrite = bool(r.random() < 0.5)
    seq_actions = max(NA, 2)
    schedules, obs = rc.random_design(r, D, n_sched, n_trials, max_len, seq_actions,
                                      arrays=overwrite or bool(r.random() < 0.5),
                                      dense=bool(r.random() < 0.5))
    schedule_of = r.integers(0, n_sched, N)

    def table(lo, hi):
        kind = int(r.integers(3))
        if kind == 0:
            return float(lo + (hi - lo) * r.random())
        shape = (D, NA) if kind == 1 else (N, D, NA)
        return {k: lo + (hi - lo) * r.random(shape) for k in KEYS}

    kw = dict(saturation=table(1.0, 5.0), learning_rate=table(0.0, 0.3),
              noise=float(r.choice([0.0, 0.5])), linear_update=bool(r.random() < 0.5))
    eps = float(r.choice([0.05, 0.2, 0.5])) if r.random() < 0.5 else 0.05 + 0.5 * r.random(N)
    eps_test = None if r.random() < 0.5 else 0.0
    sessions, left = [], n_trials
    while left > 0 and len(sessions) < 8:
        u = r.random()
        if u < 0.6 or not sessions:
            t = min(left, int(r.integers(1, max(2, left // 2 + 1))))
            kind = 'train' if (u < 0.45 or not sessions) else 'test'
            sessions.append((kind, t, int(r.integers(1, max_len + 2))))
            left -= t
        elif u < 0.72:
            sessions.append(('rescale', {'excitatory': float(r.choice([0.5, 0.9, 1.5])),
                                         'inhibitory': float(r.choice([0.5, 1.1, 1.5]))}))
        elif u < 0.84:
            sessions.append(('alpha', float(r.choice([0.25, 0.5, 2.0]))))
        else:
            sessions.append(('predict', r.random((D, D))))
    while sessions[-1][0] not in ('train', 'test'):   # (the last matrices recorded are a trial's)
        sessions.pop()
    ids = r.choice(100_000, N, replace=False)
    return dict(seed=seed, D=D, N=N, G=G, n_actions=n_actions, n_sched=n_sched, n_trials=n_trials,
                max_len=max_len, overwrite=overwrite, seq_actions=seq_actions, schedules=schedules,
                obs=obs, schedule_of=schedule_of, kw=kw, eps=eps, eps_test=eps_test,
                sessions=sessions, ids=ids)


def _kind(v) -> str:
    if type(v) is dict:
        return 'per instance' if v['excitatory'].ndim == 3 else 'table'
    return 'scalar' if np.ndim(v) == 0 else 'per instance'


def describe(c: dict) -> str:
    return ('seed %(seed)d D=%(D)d G=%(G)d N=%(N)d n_actions=%(n_actions)d schedules=%(n_sched)d '
            'trials=%(n_trials)d max_len=%(max_len)d overwrite=%(overwrite)d' % c
            + ' noise=%g linear=%d saturation=%s rate=%s epsilon=%s sessions=%s'
            % (c['kw']['noise'], c['kw']['linear_update'], _kind(c['kw']['saturation']),
               _kind(c['kw']['learning_rate']), _kind(c['eps']),
               [(s[0],) + tuple(s[1:] if s[0] in ('train', 'test') else ()) for s in c['sessions']]))


def restate_instance(c: dict, i: int, probe=None) -> dict:
    import anet_common as ac

    def mine(v):
        if type(v) is dict and v['excitatory'].ndim == 3:
            return {k: v[k][i] for k in KEYS}
        return v

    kw = dict(c['kw'], saturation=mine(c['kw']['saturation']),
              learning_rate=mine(c['kw']['learning_rate']))
    eps = c['eps'] if np.ndim(c['eps']) == 0 else float(c['eps'][i])
    return ac.restate(c['schedules'][int(c['schedule_of'][i])], c['obs'], c['seq_actions'],
                      c['overwrite'], c['n_actions'], eps, c['eps_test'], kw, c['sessions'],
                      int(c['ids'][i]), probe=probe)


def probe_of(c: dict) -> np.ndarray:
    return np.random.default_rng(99).random((c['D'], c['D']))


def run_case(c: dict) -> list:
    import anet_common as ac
    rec = ac.new_record()
    ag, env = ac.device_run(c['schedules'], c['obs'], c['seq_actions'], c['overwrite'],
                            c['n_actions'], c['eps'], c['eps_test'], c['kw'], c['sessions'],
                            n_envs=c['N'], instance_ids=c['ids'], schedule_of=c['schedule_of'],
                            rec=rec)
    N, D, NA = c['N'], c['D'], c['n_actions'] - 1
    outs = [ac.device_record(ag, env, i) for i in range(N)]
    # (one call for all instances, after the counters were read: it advances the agent's stream)
    predict = np.asarray(ag.predict_on_batch(probe_of(c)).cpu().numpy() if N > 1
                         else ag.predict_on_batch(probe_of(c))).reshape(N, D, NA)
    mid = [np.asarray(m, dtype=np.float64).reshape(N, D, NA) for m in rec['mid_predict']]
    bad = []
    for i, out in enumerate(outs):
        ref = restate_instance(c, i, probe=probe_of(c))
        out['predict'] = predict[i]
        out['mid_predict'] = np.array([m[i] for m in mid], dtype=np.float64).reshape(-1, D, NA)
        try:
            ac.assert_same_record(out, ref, what='instance %d' % i)
            assert np.array_equal(out['We_final'], ref['We'][-1]), 'instance %d: We' % i
            assert np.array_equal(out['Wi_final'], ref['Wi'][-1]), 'instance %d: Wi' % i
        except AssertionError as err:
            bad.append(str(err)[:300])
    return bad


def main() -> int:
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    failed, t0 = [], time.time()
    for seed in range(first, first + count):
        c = draw_case(seed)
        try:
            bad = run_case(c)
        except Exception as e:       # (not a mismatch: nothing more is started on the device)
            print('ERROR %s: %s' % (type(e).__name__, str(e)[:300]), describe(c), flush=True)
            return 2
        if bad:
            failed.append(seed)
            print('MISMATCH', bad[:6], describe(c), flush=True)
        if (seed - first) % 10 == 9:
            print('... %d cases, %d failing, %.0f s' % (seed - first + 1, len(failed), time.time() - t0),
                  flush=True)
    print('cases %d, failing %d: %s' % (count, len(failed), failed))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
