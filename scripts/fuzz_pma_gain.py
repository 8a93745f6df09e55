#!/usr/bin/env python3
"""Randomised parity sweep for PMAMemory's observables on the device (csrc/pma_gain.hip:
``compute_gain_batch``, ``compute_gain``, ``action_probs_batch``, ``update_q``) against the NumPy
restatement (tests/pma_common.py), bit for bit.

    python scripts/fuzz_pma_gain.py [first_seed] [count]

A case: a random successor table ``next[S, A]`` with up to 40 states and 1 .. 8 actions, 1 .. 5
instances each filled by its own random stores (self-loops, terminal transitions, repeated
experiences), a random action mask that leaves every state an action, random switches (both gain
modes, three values of ``min_gain``, learning rate, ``gamma`` and ``gamma_q``, epsilon), Q tables with
one decimal (exact ties abound), all zero or continuous, shared or one per instance, and random
sequences of 1 .. 40 steps, shared or one per instance.  tests/test_gpu_fuzz_pma_gain.py runs a
fixed slice; tests/test_host_fuzz_pma_gain.py says what that slice contains.
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

SEED = 0xC0BE1
KEYS = ('state', 'action', 'reward', 'next_state', 'terminal')


# -- cases ----------------------------------------------------------------------------------------
def draw_case(seed: int) -> dict:
    r = np.random.default_rng(seed)
    A = int(r.integers(1, 9))
    S = int(r.choice([1, 2, 3, 7, 8, 9, 16, 17, 25, 32, 33, 40]))
    n = int(r.choice([1, 2, 5]))
    nxt = r.integers(0, S, (S, A))
    nxt = np.where(r.random((S, A)) < 0.15, np.arange(S)[:, None], nxt)
    mask = r.random((S, A)) < 0.7
    mask[np.arange(S), r.integers(0, A, S)] = True
    rewards = [1.0, -1.0, 0.0, 0.0, 0.5, 10.0, -0.25]

    def experience(s=None):
        s = int(r.integers(S)) if s is None else s
        a = int(r.integers(A))
        ns = int(nxt[s, a]) if r.random() < 0.9 else int(r.integers(S))
        return [s, a, float(r.choice(rewards)), ns, int(r.random() >= 0.1)]

    stores = []
    for _ in range(n):
        rows, s = [], int(r.integers(S))
        for _ in range(int(r.integers(3, 41))):
            e = list(rows[-1]) if rows and r.random() < 0.15 else experience(s)
            rows.append(e)
            s = int(r.integers(S)) if e[4] == 0 else e[3]
        stores.append(rows)

    def table(shape):
        kind = r.random()
        if kind < 0.1:
            return np.zeros(shape)
        if kind < 0.6:
            return np.round(r.normal(size=shape), 1)
        return r.normal(size=shape) * float(r.choice([1.0, 10.0]))

    def sequence():
        length = int(r.choice([1, 1, 2, 3, 5, 8, 13, 40]))
        rows, s = [], int(r.integers(S))
        live = r.random() < 0.6                       # no terminal step but perhaps the last
        for j in range(length):
            e = experience(s)
            if live:
                e[4] = 1
            rows.append(e)
            s = e[3]
        return rows

    n_seq = int(r.integers(1, 5))
    per_seq = bool(n > 1 and r.random() < 0.5)
    seqs = [[sequence() for _ in range(n)] if per_seq else sequence() for _ in range(n_seq)]
    per_upd = bool(n > 1 and r.random() < 0.5)
    updates = [[sequence() for _ in range(n)] if per_upd else sequence() for _ in range(3)]
    return dict(seed=seed, S=S, A=A, n=n, base=int(r.integers(0, 1000)), next=nxt, mask=mask,
                masked=bool(r.random() < 0.5), stores=stores,
                gamma=float(r.choice([0.5, 0.9, 0.99])), gamma_q=float(r.choice([0.9, 0.99])),
                eps=float(r.choice([0.0, 0.1, 0.3])), lrq=float(r.choice([0.9, 0.5, 1.0])),
                min_gain=float(r.choice([10 ** -6, 1e-3, 0.1])),
                mode=str(r.choice(['original', 'other'])),
                Q=table((n, S, A) if r.random() < 0.6 else (S, A)), Q_update=table((n, S, A)),
                per_seq=per_seq, seqs=seqs, per_upd=per_upd, updates=updates,
                prob_rows=int(r.choice([1, 5, 63, 64, 65, 130])),
                wide=bool(r.random() < 0.25))


def describe(c: dict) -> str:
    lens = [[len(u) for u in s] if c['per_seq'] else len(s) for s in c['seqs']]
    return ('seed %(seed)d S=%(S)d A=%(A)d n=%(n)d base=%(base)d wide=%(wide)d masked=%(masked)d '
            'gamma=%(gamma)g gamma_q=%(gamma_q)g eps=%(eps)g lrq=%(lrq)g min_gain=%(min_gain)g '
            'mode=%(mode)s' % c + ' Q%s sequences=%s' % (list(c['Q'].shape), lens))


def exp(row) -> dict:
    return {'state': int(row[0]), 'action': int(row[1]), 'reward': float(row[2]),
            'next_state': int(row[3]), 'terminal': int(row[4])}


def _q(c, i):
    return c['Q'][i] if c['Q'].ndim == 3 else c['Q']


def _mine(c, per, seq, i):
    return [exp(r) for r in (seq[i] if per else seq)]


def prob_table(c):
    r = np.random.default_rng(c['seed'] + 77)
    rows, A = c['prob_rows'], c['A']
    q = np.round(r.normal(size=(rows, A)), 1)
    mask = None
    if c['masked']:
        mask = r.random((rows, A)) < 0.6
        mask[np.arange(rows), r.integers(0, A, rows)] = True
    return q, mask


# -- the restatement alone --------------------------------------------------------------------------
def run_reference(c: dict):
    """-> (values, facts): what the restatement makes of the case, and what the case held — tied
    rows, clipped and unclipped gains, an ``update_q`` that broke early."""
    import pma_common as pc
    from oracle.ref_loop import RefEpsilonGreedy
    n, mask = c['n'], c['mask'] if c['masked'] else None
    sas = pc.sas_of(c['next'])
    mems = []
    for i in range(n):
        m = pc.RefPMAMemory(sas, RefEpsilonGreedy(c['eps'], None), learning_rate_q=c['lrq'],
                            gamma=c['gamma'], gamma_q=c['gamma_q'])
        m.min_gain, m.min_gain_mode = c['min_gain'], c['mode']
        for row in c['stores'][i]:
            m.store(exp(row))
        mems.append(m)
    batch = np.array([m.compute_gain_batch(np.array(_q(c, i)), mask) for i, m in enumerate(mems)])
    seq = np.array([[m.compute_gain(_q(c, i), mask, _mine(c, c['per_seq'], s, i)) for s in c['seqs']]
                    for i, m in enumerate(mems)], dtype=np.float64)
    updated, broke = [], 0
    for u in c['updates']:
        rows = []
        for i, m in enumerate(mems):
            before = np.array(c['Q_update'][i])
            mine = _mine(c, c['per_upd'], u, i)
            after = m.update_q(np.array(before), mine)
            broke += int(len(mine) > 1 and any(e['terminal'] == 0 for e in mine)
                         and np.array_equal(before, after))
            rows.append(after)
        updated.append(np.array(rows))
    q, pmask = prob_table(c)
    probs = mems[0]._probs_batch(q, pmask)
    tables = np.asarray(c['Q']).reshape(-1, c['A'])
    tied = (tables == tables.max(axis=1, keepdims=True)).sum(axis=1) > 1
    facts = {'tied_rows': int(tied.sum()) if c['A'] > 1 else 0,
             'clipped': int((batch == c['min_gain']).sum()), 'unclipped': int((batch > c['min_gain']).sum()),
             'mode': c['mode'], 'broke': broke}
    return {'batch': batch, 'seq': seq, 'updated': updated, 'probs': probs}, facts


# -- the device against it --------------------------------------------------------------------------
def _stack(c, per, seq):
    """One update for the device: experience dicts of scalars, or of [N] arrays with -1 past the
    end of an instance's sequence."""
    if not per:
        return [exp(r) for r in seq]
    none = [-1, 0, 0.0, 0, 1]
    longest = max(len(u) for u in seq)
    cols = [[(u[j] if j < len(u) else none) for u in seq] for j in range(longest)]
    return [{k: [row[x] for row in col] for x, k in enumerate(KEYS)} for col in cols]


def run_case(c: dict) -> list:
    import torch
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    import pma_common as pc
    want, _ = run_reference(c)
    n, mask = c['n'], c['mask'] if c['masked'] else None
    mem = PMAMemory(pc.sas_of(c['next']), EpsilonGreedy(c['eps']), learning_rate_q=c['lrq'],
                    gamma=c['gamma'], gamma_q=c['gamma_q'], wide=c['wide'])
    mem.min_gain, mem.min_gain_mode = c['min_gain'], c['mode']
    mem.bind(n, seed=SEED, instance_base=c['base'])
    none = {'state': -1, 'action': 0, 'reward': 0.0, 'next_state': 0, 'terminal': 1}
    for k in range(max(len(rows) for rows in c['stores'])):
        pick = [exp(rows[k]) if k < len(rows) else none for rows in c['stores']]
        mem.store({key: [e[key] for e in pick] for key in KEYS})
    mem.counter.fill_(11)
    mem._policy_counter().fill_(13)
    host = lambda x: x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)   # noqa: E731
    bad = []

    def cmp(name, got, ref):
        got, ref = host(got).reshape(np.shape(ref)), np.asarray(ref)
        if not np.array_equal(got, ref):
            at = np.argwhere(got != ref)[0].tolist()
            bad.append('%s at %s: %r != %r' % (name, at, got[tuple(at)], ref[tuple(at)]))

    cmp('compute_gain_batch', mem.compute_gain_batch(c['Q'], mask), want['batch'])
    cmp('compute_gain', mem.compute_gain(c['Q'], mask, [_stack(c, c['per_seq'], s) for s in c['seqs']]),
        want['seq'])
    for k, u in enumerate(c['updates']):
        q = torch.as_tensor(np.array(c['Q_update']), device=mem.device)
        mem.update_q(q, _stack(c, c['per_upd'], u))
        cmp('update_q %d' % k, q, want['updated'][k])
    q, pmask = prob_table(c)
    cmp('action_probs_batch', mem.action_probs_batch(q, pmask), want['probs'])
    if not (bool((mem.counter == 11).all()) and bool((mem.policy.counter == 13).all())):
        bad.append('a counter moved')
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
