"""``PMAMemory.compute_gain_batch`` and ``PMA.update_q`` on the device against the only alternative
the parent had (docs/MEASUREMENTS.md §30): the NumPy restatement of ``compute_gain_batch`` looping
over the instances, and ``PMA.update_q``'s host loop (download every Q, loop in Python, upload), on
the CPU of the same box.

Open fields of 5 x 5 (25 states) and 32 x 32 (1 024 states, a wide memory), four actions, 1 and
1 024 instances, every memory filled by 40 stores per instance.  Device calls: the median of
``--reps`` calls timed one by one between ``torch.cuda.synchronize()`` brackets by the host clock
(what a caller waits for, allocations and the result's download for one instance included), after
two warm-up calls, and the kernel alone from events around the C entry point on preallocated
tensors.  The restatement is timed on ``--cpu-instances`` instances at most and scaled to the
instance count (it is one independent Python loop per instance); ``update_q`` applies a seven-step
sequence.  The results are compared before anything is timed.

    python scripts/experiments/pma_gain/time_gain.py [--reps 20] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
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
from oracle.ref_loop import RefEpsilonGreedy  # noqa: E402

STORES = 40


def world_of(side):
    from cobel_amd.misc.gridworld_tools import make_open_field
    return make_open_field(side, side, 0, 1)


def wall(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e6, float(np.min(times)) * 1e6, float(np.max(times)) * 1e6


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def configuration(side, n, reps, cpu_instances):
    from cobel_amd import _lib as L
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = world_of(side)
    tabs, sas = pc.tables_of(world)
    S, A = np.asarray(tabs['next']).shape
    wide = S > L.PMA_MAX_STATES
    env = Gridworld(world, n_envs=n, seed=2024)
    mem = PMAMemory(sas, EpsilonGreedy(0.1), gamma_q=0.99, wide=wide)
    agent = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    agent._bind(env)
    k = min(n, cpu_instances)
    walks = [pc.walk_stores(tabs, STORES, seed=i + 1) for i in range(k)]
    for j in range(STORES):
        pick = [walks[i % k][j] for i in range(n)]
        mem.store({'state': [r[0] for r in pick], 'action': [r[1] for r in pick],
                   'reward': [r[2] for r in pick], 'next_state': [r[3] for r in pick],
                   'terminal': [r[4] for r in pick]})
    Q = np.random.default_rng(5).normal(size=(n, S, A))
    Qd = torch.as_tensor(Q, device=mem.device)
    agent.Q = Qd
    update = [dict(zip(pc.KEYS, (r[0], r[1], r[2], r[3], 1))) for r in walks[0][:7]]
    out = {'states': S, 'actions': A, 'instances': n, 'wide': wide, 'cpu_instances': k}

    # -- compute_gain_batch -----------------------------------------------------------------------
    refs = []
    for i in range(k):
        ref = pc.RefPMAMemory(sas, RefEpsilonGreedy(0.1, None), gamma_q=0.99)
        for r in walks[i]:
            ref.store(dict(zip(pc.KEYS, r)))
        refs.append(ref)
    t0 = time.perf_counter()
    want = np.array([refs[i].compute_gain_batch(Q[i], None) for i in range(k)])
    cpu = (time.perf_counter() - t0) / k
    got = mem.compute_gain_batch(Qd, None)
    got = got if n == 1 else got[:k].cpu().numpy()
    assert np.array_equal(got.reshape(want.shape), want), 'device and restatement differ'
    med, lo, hi = wall(lambda: mem.compute_gain_batch(Qd, None), reps)
    gain = torch.empty((n, A * S), dtype=torch.float64, device=mem.device)
    m = mem._mem()
    stream = L.current_stream(mem.device)
    kern = events(lambda: L.check(L.lib().cobel_pma_gain_batch(
        C.byref(m), L.ptr(Qd), S * A, L.ptr(gain), stream)), reps)
    out['compute_gain_batch'] = {
        'device_call_us': med, 'device_call_min_us': lo, 'device_call_max_us': hi,
        'device_kernel_us': kern, 'restatement_us_per_instance': cpu * 1e6,
        'restatement_us_all_instances': cpu * 1e6 * n, 'restatement_timed_on': k}

    # -- PMA.update_q -----------------------------------------------------------------------------
    before = agent._q.clone()
    agent.update_q(update)
    dev = agent._q.cpu().numpy()
    agent._q.copy_(before)
    view = _HostView(agent)
    PMA.update_q(view, update)
    assert np.array_equal(view.result.reshape(dev.shape), dev), 'device and host loop differ'
    med, lo, hi = wall(lambda: agent.update_q(update), reps)
    cpu_times = []
    for _ in range(3):
        agent._q.copy_(before)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = _HostView(agent)
        PMA.update_q(v, update)
        agent._q.copy_(torch.as_tensor(v.result.reshape(dev.shape), device=mem.device))
        torch.cuda.synchronize()
        cpu_times.append(time.perf_counter() - t0)
    out['update_q'] = {'steps': len(update), 'device_call_us': med, 'device_call_min_us': lo,
                       'device_call_max_us': hi, 'host_loop_us': float(np.median(cpu_times)) * 1e6}
    return out


class _HostView:
    """The parent's ``PMA.update_q`` on a bound agent's tables: what its ``Q`` getter and setter did
    (download every instance's Q, run the loop, hand the result back), with ``_q`` hidden so that
    the method takes its host loop."""

    def __init__(self, agent):
        self._agent, self._q, self.result = agent, None, None
        self.n_states, self.n_actions, self.n_envs = agent.n_states, agent.n_actions, agent.n_envs
        self.learning_rate, self.gamma = agent.learning_rate, agent.gamma

    @property
    def Q(self):
        return self._agent._q if self.result is None else self.result

    @Q.setter
    def Q(self, value):
        self.result = np.asarray(value)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cpu-instances', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    rows = []
    for side in (5, 32):
        for n in (1, 1024):
            rows.append(configuration(side, n, args.reps, args.cpu_instances))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
