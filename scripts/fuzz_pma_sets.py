#!/usr/bin/env python3
"""Randomised parity sweep for PMA's per-instance parameter sets: ``PMA.train`` on the device with
array-valued parameters (cobel_pma_trial, cobel_pma_update_sr and cobel_pma_replay with
``param_index``) against the NumPy restatement (tests/pma_common.py) run with each instance's own
ten values, bit for bit, nothing injected: the device runs its own ``update_sr``, the restatement
``pma_common.gauss_jordan``.

    python scripts/fuzz_pma_sets.py [first_seed] [count]

Per seed: a seeded gridworld of 4 .. 42 states, 1 .. 5 parameter sets whose ten values are drawn
(every set has a learning rate of the agent of its own, so no two sets act alike), 3 .. 12
instances spread over them, a shared or a separate memory policy, masked actions or not, one or
two sessions; every session starts from a seeded Q table.  Three instances are re-run by the
restatement and compared: escape latencies, ``last``, every replay record, Q, the memory's tables,
SR and the four stream indices.  tests/test_gpu_fuzz_pma_sets.py runs a fixed slice,
tests/test_host_pma_sets.py says what that slice contains.  scripts/fuzz_pma.py sweeps the scalar
launches.
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
BASE_SET = dict(learning_rate=0.9, learning_rate_q=0.9, learning_rate_T=0.9, gamma=0.9,
                gamma_q=0.99, min_gain=1e-6, memory_epsilon=0.1, alpha=0.9, agent_gamma=0.99,
                epsilon=0.1)
CHOICES = dict(learning_rate=[0.3, 0.5, 1.0], learning_rate_q=[0.3, 0.6, 1.0],
               learning_rate_T=[0.1, 0.5, 0.7], gamma=[0.5, 0.8, 0.99],
               gamma_q=[0.5, 0.9, 0.95], min_gain=[1e-4, 1e-3, 0.1],
               memory_epsilon=[0.05, 0.2, 0.3], agent_gamma=[0.5, 0.9, 0.95],
               epsilon=[0.05, 0.2, 0.3])
ALPHAS = (0.3, 0.5, 0.6, 0.7, 0.8, 1.0)       # one per set, all different
BUDGET = 6_000          # policy evaluations of the restatement per instance: S x A x replayed updates


def draw_case(seed: int) -> dict:
    r = np.random.default_rng(7_000_003 * seed + 11)
    h, w = int(r.integers(2, 7)), int(r.integers(2, 8))
    S = h * w
    goal = int(r.integers(S))
    walls = []
    for _ in range(int(r.integers(0, max(1, S // 4)))):
        a = int(r.integers(S))
        b = a + int(r.choice([-1, 1, -w, w]))
        if 0 <= b < S and not (abs(b - a) == 1 and a // w != b // w):
            walls += [(a, b), (b, a)]
    n = int(r.choice([3, 7, 12]))
    n_sets = int(r.choice([1, 2, 3, 5]))
    alphas = [float(a) for a in r.permutation(ALPHAS)[:n_sets]]
    sets = []
    for k in range(n_sets):
        s = dict(BASE_SET, alpha=alphas[k])
        for name, values in CHOICES.items():
            if r.random() < 0.5:
                s[name] = float(r.choice(values))
        sets.append(s)
    which = [int(x) for x in r.integers(0, n_sets, n)]
    which[0], which[-1] = 0, n_sets - 1
    sessions, left = [], BUDGET
    for _ in range(1 + int(r.random() < 0.4)):
        batch, trials = int(r.integers(1, 9)), int(r.integers(1, 4))
        steps = int(r.choice([2, 5, 20, 40]))
        no_replay = bool(r.random() < 0.15)
        if not no_replay:          # two replays per trial
            batch = max(1, min(batch, left // (2 * S * 4)))
            trials = max(1, min(trials, left // (2 * S * 4 * batch)))
            left = max(0, left - 2 * S * 4 * batch * trials)
        sessions.append((trials, steps, batch, no_replay))
    picks = sorted({0, n // 2, n - 1})
    return dict(seed=seed, h=h, w=w, S=S, goal=goal, walls=walls,
                reward=float(r.choice([10.0, 1.0, 2.0, -1.0])), n=n, base=int(r.integers(0, 1000)),
                sets=sets, which=which, shared=bool(r.random() < 0.4), masked=bool(r.random() < 0.5),
                sessions=sessions, picks=picks)


def describe(c: dict) -> str:
    varied = sorted({k for s in c['sets'] for k in s if s[k] != BASE_SET[k]})
    return ('seed %(seed)d %(h)dx%(w)d goal=%(goal)d n=%(n)d base=%(base)d shared=%(shared)d '
            'masked=%(masked)d sessions=%(sessions)s which=%(which)s' % c
            + ' sets=%d varied=%s walls=%d' % (len(c['sets']), varied, len(c['walls']) // 2))


def make_world(c: dict):
    from cobel_amd.misc.gridworld_tools import make_gridworld
    return make_gridworld(c['h'], c['w'], terminals=[c['goal']],
                          rewards=np.array([[c['goal'], c['reward']]]), goals=[c['goal']],
                          invalid_transitions=list(c['walls']))


def q_start(c: dict) -> np.ndarray:
    return np.random.default_rng(c['seed'] + 99).random((c['S'], 4))


def columns(c: dict) -> dict:
    return {k: np.array([c['sets'][s][k] for s in c['which']]) for k in BASE_SET}


# -- the restatement alone --------------------------------------------------------------------------
def run_reference(c: dict, instance: int, params: dict) -> dict:
    """What the restatement makes of global instance ``c['base'] + instance`` under ``params``."""
    import pma_common as pc
    from oracle.philox import STREAM_ENV, STREAM_POLICY, TapeRNG
    from oracle.ref_loop import RefEpsilonGreedy, RefGridworld
    tabs = make_world(c).compact()
    sas = pc.sas_of(tabs['next'])
    inst = c['base'] + instance
    env = RefGridworld(tabs, TapeRNG(SEED, inst, STREAM_ENV))
    rm, rp = pc.memory_rngs(SEED, inst)
    pol = RefEpsilonGreedy(params['epsilon'], TapeRNG(SEED, inst, STREAM_POLICY))
    mem = pc.RefPMAMemory(sas, pol if c['shared'] else RefEpsilonGreedy(params['memory_epsilon'], rp),
                          learning_rate=params['learning_rate'],
                          learning_rate_q=params['learning_rate_q'], gamma=params['gamma'],
                          gamma_q=params['gamma_q'], rng=rm, sr_by_elimination=True)
    mem.learning_rate_T, mem.min_gain = params['learning_rate_T'], params['min_gain']
    agent = pc.RefPMA(c['S'], 4, pol, mem, learning_rate=params['alpha'], gamma=params['agent_gamma'])
    agent.Q = q_start(c)
    if c['masked']:
        agent.mask_actions, agent.action_mask = True, pc.masked_actions(tabs)
    tr = pc.new_trace()
    for trials, steps, batch, no_replay in c['sessions']:
        agent.train(env, trials, steps, batch, no_replay, trace=tr)
    return {'steps': np.array(tr['steps']), 'replay_start': tr['replay_start'],
            'replay_end': tr['replay_end'], 'last': tr['last'][-1], 'Q': agent.Q, 'T': mem.T,
            'SR': mem.SR, 'rewards': mem.rewards, 'states': mem.states, 'terminals': mem.terminals,
            'index': [env.rng.index, agent.policy.rng.index, mem.rng.index, mem.policy.rng.index]}


def sets_act_differently(c: dict) -> bool:
    """The condition a case must meet to say anything about sets: the restatement's final Q of
    ONE instance differs between every two sets of the case — a kernel that gave every instance
    set 0 could not pass."""
    qs = [run_reference(c, c['picks'][0], s)['Q'] for s in c['sets']]
    return all(not np.array_equal(qs[a], qs[b]) for a in range(len(qs)) for b in range(a))


# -- the device against it --------------------------------------------------------------------------
def run_case(c: dict) -> list:
    import pma_common as pc
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    n, cols = c['n'], columns(c)
    world = make_world(c)
    tabs = world.compact()
    env = Gridworld(world, n_envs=n, seed=SEED, instance_base=c['base'])
    pol = EpsilonGreedy(cols['epsilon'])
    mem = PMAMemory(pc.sas_of(tabs['next']),
                    pol if c['shared'] else EpsilonGreedy(cols['memory_epsilon']),
                    learning_rate=cols['learning_rate'], learning_rate_q=cols['learning_rate_q'],
                    gamma=cols['gamma'], gamma_q=cols['gamma_q'])
    mem.learning_rate_T, mem.min_gain = cols['learning_rate_T'], cols['min_gain']
    seen = []
    agent = PMA(env.observation_space, env.action_space, pol, mem,
                learning_rate=cols['alpha'], gamma=cols['agent_gamma'], custom_callbacks={
                    'on_replay_end': [lambda logs: seen.append([pc.rows_of(u) for u in logs['replay']])]})
    agent.Q = q_start(c)
    if c['masked']:
        agent.mask_actions, agent.action_mask = True, pc.masked_actions(tabs)
    agent.track_instances = True
    for trials, steps, batch, no_replay in c['sessions']:
        agent.train(env, trials, steps, batch, no_replay)
    bad = []

    def cmp(name, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        if got.shape != ref.shape or not np.array_equal(got, ref):
            bad.append(name)

    q, last = agent.Q.cpu().numpy(), agent._last.cpu().numpy()
    lat = agent.monitors.lat_trace.cpu().numpy()
    for i in c['picks']:
        want = run_reference(c, i, c['sets'][c['which'][i]])
        total = len(want['steps'])
        cmp('lat_trace of %d' % i, lat[i][:total], want['steps'])
        cmp('replays of %d' % i, len(seen), len(want['replay_start']) + len(want['replay_end']))
        for k, (a, b) in enumerate(zip(seen[0::2], want['replay_start'])):
            cmp('replay at the start of replayed trial %d of %d' % (k, i), a[i], b)
        for k, (a, b) in enumerate(zip(seen[1::2], want['replay_end'])):
            cmp('replay at the end of replayed trial %d of %d' % (k, i), a[i], b)
        cmp('Q of %d' % i, q[i], want['Q'])
        cmp('last of %d' % i, last[i], want['last'])
        for name in ('T', 'SR', 'rewards', 'states', 'terminals'):
            cmp('%s of %d' % (name, i), np.asarray(getattr(mem, name))[i], want[name])
        cmp('index of %d' % i,
            [int(env.env_ctr[i].item()), int(agent.policy.counter[i].item()),
             int(mem.counter[i].item()), int(mem.policy.counter[i].item())], want['index'])
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
