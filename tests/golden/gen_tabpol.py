"""Golden traces of QAgent and DynaQ with the reference's Softmax, ExclusiveEpsilonGreedy and
RandomDiscrete policies, recorded from the real reference.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_tabpol.py

Reuses the shim and the tape generators of gen_golden.py; the cases and worlds are
tests/tabpol_common.py's.  The reference's classes run unchanged on the build's Philox tapes, with
the two coercions BASELINE.md lists: the tables are float32 (as gen_golden.py coerces them), and
``Softmax`` is handed the row promoted to float64 (the reference's Softmax computes in the dtype of
the row it is given, and NumPy's float32 ``exp`` is a SIMD routine no device code reproduces).

A case is kept only if every uniform draw lies at least 1e-9 from every edge of the CDF it is
compared with (tests/golden/gen_qseq.py's rule: the device's ``exp`` and its sum of eight
exponentials differ from NumPy's in the last bits); otherwise the generator stops and the case
takes another instance number.  The worst margin of a case is stored with it.

Writes tabpol_traces.npz: per case the per-step (state, action, reward, next state, non-terminal,
td), per trial ``logs['steps']``, ``logs['trial_reward']`` and Q, the final Q, Dyna-Q's model /
QAgent's log as packed words, the draws each tape handed out, and the compact world tables.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import (SEED, STREAM_ENV, STREAM_MEMORY, STREAM_POLICY, DynaQ,  # noqa: E402
                        EpsilonGreedy, Gridworld, QAgent, TapeRNG, gt)

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
import tabpol_common as tc  # noqa: E402

from cobel.interface import Topology  # noqa: E402
from cobel.misc import topology_tools as tt  # noqa: E402
from cobel.policy.greedy import ExclusiveEpsilonGreedy  # noqa: E402
from cobel.policy.random import RandomDiscrete  # noqa: E402
from cobel.policy.softmax import Softmax  # noqa: E402
from oracle.philox import STREAM_AUX  # noqa: E402  (the stream of a policy_test of its own)

assert SEED == tc.SEED


class Softmax64(Softmax):
    def get_action_probs(self, v, mask=None):
        return super().get_action_probs(np.asarray(v, dtype=np.float64), mask)


def make_policy(spec, rng, n_actions, margin):
    kind, par = spec
    if kind == tc.RANDOM:
        return RandomDiscrete(n_actions, rng=rng)
    pol = {tc.SOFTMAX: Softmax64, tc.EXCLUSIVE: ExclusiveEpsilonGreedy, 'eps': EpsilonGreedy}[kind](
        par, rng=rng)
    real = pol.select_action

    def select(v, mask=None):      # the margin between the draw and the edges of its CDF
        a = real(v, mask)
        cdf = np.cumsum(pol.get_action_probs(v, mask))
        cdf /= cdf[-1]
        if len(cdf) > 1:
            margin[0] = min(margin[0], float(np.abs(cdf[:-1] - pol.rng.log[-1]).min()))
        return a
    pol.select_action = select
    return pol


def run_case(name) -> dict:
    c = tc.case(name)
    opt, inst = c['opt'], c['inst']
    rng = TapeRNG(SEED, inst, STREAM_ENV)
    if c['world'] == 'hex':
        nodes, starts = tc.hex_nodes(tt)
        env = Topology(nodes, starts, None, rng=rng)
        tabs = tc.node_tables(nodes, starts)
        keys = [tuple(np.array(nodes[k]['pose']).flatten()) for k in nodes]
    else:
        world = tc.grid4(gt)
        env = Gridworld(world, rng=rng)
        tabs = tc.world_tables(world)
        keys = [(s,) for s in range(int(world['states']))]
    S, A = tabs['next'].shape
    margin = [float('inf')]
    pol = make_policy(c['policy'], TapeRNG(SEED, inst, STREAM_POLICY), A, margin)
    pol_test = None
    if opt.get('test'):
        pol_test = make_policy(opt['test'], TapeRNG(SEED, inst, STREAM_AUX), A, margin)
    mem = TapeRNG(SEED, inst, STREAM_MEMORY)
    if c['agent'] == 'dynaq':
        ag = DynaQ(env.observation_space, env.action_space, pol, pol_test)
        ag.M.rng = mem
        ag.Q = ag.Q.astype(np.float32)
        ag.M.rewards = ag.M.rewards.astype(np.float32)
        if opt.get('mask'):
            ag.mask_actions, ag.action_mask = True, tc.two_action_mask(tabs['next'])
        table = lambda: np.array(ag.Q, dtype=np.float32)       # noqa: E731
    else:
        ag = QAgent(env.observation_space, env.action_space, pol, pol_test, rng=mem)
        for k in keys:      # float32 rows (created lazily as float64 otherwise)
            ag.Q[k] = np.zeros(A, dtype=np.float32)
        table = lambda: np.array([ag.Q[k] for k in keys], dtype=np.float32)       # noqa: E731
    index = {k: i for i, k in enumerate(keys)}
    first = lambda x: x if isinstance(x, tuple) else (int(x),)       # noqa: E731
    sarsn, tds, steps_log, rewards, q_trial = [], [], [], [], []

    def on_step_end(logs):
        sarsn.append((index[first(logs['state'])], logs['action'], logs['reward'],
                      index[first(logs['next_state'])], logs['terminal']))
        td = logs.get('td', 0.0)
        tds.append(float(td) if np.ndim(td) == 0 else 0.0)

    def on_trial_end(logs):
        steps_log.append(logs['steps'])
        rewards.append(float(logs['trial_reward']))
        q_trial.append(table())

    ag.callbacks.custom_callbacks = {'on_step_end': [on_step_end], 'on_trial_end': [on_trial_end],
                                     'on_trial_begin': [], 'on_step_begin': []}
    if c['agent'] == 'dynaq':
        ag.train(env, tc.TRIALS, tc.STEPS, c['batch'], bool(opt.get('no_replay')))
    else:
        ag.train(env, tc.TRIALS, tc.STEPS, c['batch'])
    n_train = len(sarsn)
    if opt.get('test'):
        ag.test(env, tc.TRIALS, tc.STEPS)
    assert table().dtype == np.float32
    a = np.array(sarsn, dtype=np.float64).reshape(-1, 5)
    d = dict(state=a[:, 0].astype(np.int16), action=a[:, 1].astype(np.int8), reward=a[:, 2],
             next_state=a[:, 3].astype(np.int16), nonterminal=a[:, 4].astype(np.int8),
             td=np.array(tds, dtype=np.float64), steps=np.array(steps_log, dtype=np.int32),
             trial_reward=np.array(rewards, dtype=np.float64), Q_trial=np.array(q_trial, dtype=np.float32),
             Q=table(), ctr_env=np.int64(env.rng.index), ctr_policy=np.int64(pol.rng.index),
             ctr_policy_test=np.int64(0 if pol_test is None else pol_test.rng.index),
             ctr_memory=np.int64(mem.index), margin=np.float64(margin[0]),
             n_train_steps=np.int64(n_train))
    if c['agent'] == 'dynaq':
        assert ag.M.rewards.dtype == np.float32
        d.update(M_rewards=np.array(ag.M.rewards, dtype=np.float32),
                 M_states=ag.M.states.astype(np.int16), M_terminals=ag.M.terminals.astype(np.int8))
    else:
        d['log'] = tc.pack_log([(index[first(e['state'])], e['action'], e['reward'],
                                 index[first(e['next_state'])], e['terminal']) for e in ag.M], A)
    for k in ('next', 'reward', 'terminal', 'starts'):
        d['world/' + k] = tabs[k]
    if opt.get('mask'):
        d['action_mask'] = tc.two_action_mask(tabs['next'])
    return d


def policy_rows() -> dict:
    """get_action_probs of the reference's Softmax (float64 rows) and ExclusiveEpsilonGreedy (float32
    rows on a half-integer grid: ties) on seeded random rows of one to eight values, some masked."""
    r = np.random.default_rng(20261021)
    n = 240
    v = np.full((n, 8), np.nan)
    vq = np.full((n, 8), np.nan, dtype=np.float32)
    soft, excl = np.full((n, 8), np.nan), np.full((n, 8), np.nan)
    A = np.zeros(n, dtype=np.int8)
    bits = np.zeros(n, dtype=np.uint8)
    beta, eps = np.zeros(n), np.zeros(n)
    for k in range(n):
        a = 1 + k % 8
        row = r.normal(size=a)
        mask = None
        if k % 3 == 2:
            mask = r.random(a) < 0.6
            mask[r.integers(a)] = True
        A[k], beta[k], eps[k] = a, r.choice([1e-3, 0.5, 2.0, 5.0]), r.choice([0.0, 0.1, 0.3, 1.0])
        bits[k] = (1 << a) - 1 if mask is None else sum(int(b) << j for j, b in enumerate(mask))
        v[k, :a], vq[k, :a] = row, (np.round(row * 2) / 2).astype(np.float32)
        soft[k, :a] = Softmax(beta[k]).get_action_probs(row.copy(), mask)
        excl[k, :a] = ExclusiveEpsilonGreedy(eps[k]).get_action_probs(vq[k, :a].copy(), mask)
    return dict(v=v, vq=vq, A=A, bits=bits, beta=beta, eps=eps, soft=soft, excl=excl)


def main() -> None:
    out = {'rows/' + k: a for k, a in policy_rows().items()}
    for name in tc.CASES:
        d = run_case(name)
        assert d['margin'] > tc.MARGIN, '%s: a draw within 1e-9 of an edge of its CDF (%g): take ' \
                                        'another instance number' % (name, d['margin'])
        print('%-22s steps %4d margin %.3g' % (name, len(d['state']), d['margin']))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    path = G._out('tabpol_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
