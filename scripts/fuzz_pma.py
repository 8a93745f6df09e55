#!/usr/bin/env python3
"""Randomised parity sweep for PMA: PMAMemory and the PMA agent on the device (csrc/pma.hip,
csrc/pma_sr.hip) against the NumPy restatement (tests/pma_common.py), bit for bit, with nothing
injected: the device runs its own ``update_sr``, the restatement ``pma_common.gauss_jordan``.

    python scripts/fuzz_pma.py [first_seed] [count]

Seeds below 10^6 are memory cases: a random successor table ``next[S, A]`` with 1 .. 8 actions
(self-loops, absorbing states), narrow and wide sizes, a walk of stores with a random script of
``update_sr``, replays (from a state, from ``None``, forced first, masked), ``mask`` and switch
flips in between; 1 .. 65 instances, one of them compared.  Seeds from 10^6 on are agent cases:
``PMA.train`` on a seeded gridworld of random shape, one or two sessions.  tests/test_gpu_fuzz_agents.py
runs a fixed slice; tests/test_host_fuzz_agents.py says what that slice contains.

The restatement evaluates the policy S x A times per replayed update, so every case has a budget of
``BUDGET`` such evaluations (S x A x length summed over its replays): replays are shortened, then
left out, once it is spent.
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
AGENT_SEEDS = 1_000_000
NARROW = (1, 2, 3, 7, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 127, 128)
WIDE = (129, 160, 272)
BUDGET = 24_000
# compute_need(None) is scipy.linalg.eig on the host, once per instance and twice per replay (the
# script records the need vector, the replay computes it again): replays from None are drawn only
# where n x S^3 stays below this (272^3 for one instance, 128^3 for ten)
EIG_LIMIT = 2.2e7
SWITCH_VALUES = {'min_gain': (10 ** -6, 1e-3, 0.1), 'min_gain_mode': ('original', 'other')}


# -- cases ----------------------------------------------------------------------------------------
def draw_case(seed: int) -> dict:
    return _draw_agent(seed) if seed >= AGENT_SEEDS else _draw_memory(seed)


def _draw_memory(seed: int) -> dict:
    r = np.random.default_rng(seed)
    A = int(r.integers(1, 9))
    wide = bool(r.random() < 0.125)
    if wide and r.random() < 0.75:
        S = int(r.choice(WIDE))
    else:                                   # (now and then a narrow size through the wide form)
        S = int(r.choice(NARROW))
    n = int(r.choice([1, 2, 5, 64, 65]))
    pick, base = int(r.integers(n)), int(r.integers(0, 1000))
    gamma, gamma_q = float(r.choice([0.5, 0.9, 0.99])), float(r.choice([0.9, 0.99]))
    eps = float(r.choice([0.1, 0.3]))
    nxt = r.integers(0, S, (S, A))
    own = np.arange(S)[:, None]
    nxt = np.where(r.random((S, A)) < 0.15, own, nxt)
    for s in r.integers(0, S, int(r.integers(0, 3))):
        nxt[s] = s                          # absorbing
    mask = r.random((S, A)) < 0.7
    mask[np.arange(S), r.integers(0, A, S)] = True
    state_flags = {'equal_need': False, 'equal_gain': False, 'ignore_barriers': True,
                   'allow_loops': False}
    max_len = 8 if wide else 33
    left = [BUDGET]
    ops, visited = [], []

    def a_state():
        if visited and r.random() < 0.7:
            return int(visited[int(r.integers(len(visited)))])
        return int(r.integers(S))

    def replay(from_state=False):
        length = int(r.integers(1, max_len + 1))
        length = min(length, left[0] // (S * A))
        if length < 1:
            return
        left[0] -= S * A * length
        u = r.random()
        state, first = a_state(), None
        if not from_state:
            if u < 0.15 and n * S ** 3 <= EIG_LIMIT:
                state = None
            if r.random() < 0.25:
                first = a_state()
        ops.append(['replay', length, state, first, bool(r.random() < 0.5)])

    def script_op():
        u = r.random()
        if u < 0.2:
            ops.append(['update_sr'])
            if r.random() < 0.7:
                replay(from_state=True)
        elif u < 0.65:
            replay()
        elif u < 0.75:
            ops.append(['mask'])
        else:
            name = str(r.choice(['equal_need', 'equal_gain', 'ignore_barriers', 'allow_loops',
                                 'min_gain', 'min_gain_mode']))
            if name in state_flags:
                state_flags[name] = not state_flags[name]
                ops.append(['set', name, state_flags[name]])
            else:
                v = SWITCH_VALUES[name][int(r.integers(len(SWITCH_VALUES[name])))]
                ops.append(['set', name, v])

    s, last = int(r.integers(S)), None
    for _ in range(int(r.integers(5, 41))):
        if last is not None and r.random() < 0.15:        # the same experience again
            e = list(last)
            if r.random() < 0.5:
                e[2] = float(r.choice([1.0, -1.0, 0.0]))
        else:
            a = int(r.integers(A))
            ns = int(nxt[s, a]) if r.random() < 0.95 else int(r.integers(S))
            e = [s, a, float(r.choice([1.0, -1.0, 0.0, 0.0, 0.5, 10.0, -0.25])), ns,
                 int(r.random() >= 0.1)]
        ops.append(['store'] + e)
        visited.append(e[0])
        last = e
        s = int(r.integers(S)) if e[4] == 0 else e[3]
        if r.random() < 0.3:
            for _ in range(int(r.integers(1, 3))):
                script_op()
    for _ in range(int(r.integers(1, 4))):
        script_op()
    replay(from_state=True)
    return dict(kind='memory', seed=seed, S=S, A=A, wide=wide, n=n, pick=pick, base=base,
                gamma=gamma, gamma_q=gamma_q, eps=eps, next=nxt, mask=mask, ops=ops)


def _draw_agent(seed: int) -> dict:
    r = np.random.default_rng(seed)
    wide = bool(r.random() < 0.08)
    h, w = (12, 11) if wide else (int(r.integers(2, 12)), int(r.integers(2, 12)))
    S = h * w
    goal = int(r.integers(S))
    walls = []
    for _ in range(int(r.integers(0, max(1, S // 4)))):
        a = int(r.integers(S))
        b = a + int(r.choice([-1, 1, -w, w]))
        if 0 <= b < S and not (abs(b - a) == 1 and a // w != b // w):
            walls += [(a, b), (b, a)]
    n = int(r.choice([1, 2, 5, 65] if S <= 36 else [1, 2, 5]))
    sessions, left = [], BUDGET
    for k in range(1 + int(r.random() < 0.5)):
        batch = int(r.integers(1, 9 if wide else 34))
        no_replay = bool(r.random() < 0.2)
        steps = int(r.choice([1, 2, 5, 20, 60, 200]))
        trials = int(r.integers(1, 5))
        if not no_replay:      # two replays per trial
            batch = max(1, min(batch, left // (2 * S * 4)))
            trials = max(1, min(trials, left // (2 * S * 4 * batch)))
            left = max(0, left - 2 * S * 4 * batch * trials)
        sessions.append((trials, steps, batch, no_replay))
    mask = None                  # 'moves': pma_common.masked_actions; an array: a random mask
    if r.random() < 0.5:
        mask = 'moves'
        if r.random() < 0.5:
            mask = r.random((S, 4)) < 0.75
            mask[np.arange(S), r.integers(0, 4, S)] = True
    return dict(kind='agent', seed=seed, h=h, w=w, S=S, A=4, wide=wide, goal=goal, walls=walls,
                reward=float(r.choice([10.0, 1.0, 2.0, -1.0])), n=n, pick=int(r.integers(n)),
                base=int(r.integers(0, 1000)), eps=float(r.choice([0.1, 0.3])),
                gamma_q=float(r.choice([0.9, 0.99])), shared=bool(r.random() < 0.3), mask=mask,
                sessions=sessions)


def describe(c: dict) -> str:
    if c['kind'] == 'memory':
        kinds = [op[0] for op in c['ops']]
        return ('seed %(seed)d memory S=%(S)d A=%(A)d wide=%(wide)d n=%(n)d pick=%(pick)d '
                'base=%(base)d gamma=%(gamma)g gamma_q=%(gamma_q)g eps=%(eps)g' % c
                + ' stores=%d replays=%s update_sr=%d'
                % (kinds.count('store'), [op[1:] for op in c['ops'] if op[0] == 'replay'],
                   kinds.count('update_sr')))
    return ('seed %(seed)d agent %(h)dx%(w)d wide=%(wide)d goal=%(goal)d n=%(n)d pick=%(pick)d '
            'base=%(base)d eps=%(eps)g gamma_q=%(gamma_q)g shared=%(shared)d sessions=%(sessions)s'
            % c + ' walls=%d mask=%s' % (len(c['walls']) // 2,
                                         c['mask'] if isinstance(c['mask'], (str, type(None))) else 'random'))


# -- the restatement alone --------------------------------------------------------------------------
def agent_world(c: dict):
    from cobel_amd.misc.gridworld_tools import make_gridworld
    return make_gridworld(c['h'], c['w'], terminals=[c['goal']],
                          rewards=np.array([[c['goal'], c['reward']]]), goals=[c['goal']],
                          invalid_transitions=list(c['walls']))


def agent_mask(c: dict, tabs):
    import pma_common as pc
    if c['mask'] is None:
        return None
    return pc.masked_actions(tabs) if isinstance(c['mask'], str) else c['mask']


def run_reference(c: dict):
    """-> (record, memory): what the restatement makes of the case."""
    import pma_common as pc
    from oracle.ref_loop import RefEpsilonGreedy
    inst = c['base'] + c['pick']
    if c['kind'] == 'memory':
        rm, rp = pc.memory_rngs(SEED, inst)
        ref = pc.RefPMAMemory(pc.sas_of(c['next']), RefEpsilonGreedy(c['eps'], rp), gamma=c['gamma'],
                              gamma_q=c['gamma_q'], rng=rm, sr_by_elimination=True)
        want = pc.ScriptMemory(ref, c['mask'],
                               index=lambda m: (m.rng.index, m.policy.rng.index)).run(c['ops'])
        return want, ref
    world = agent_world(c)
    tabs = world.compact()
    env, agent, mem = pc.make_ref_agent(tabs, pc.sas_of(tabs['next']), SEED, inst,
                                        gamma_q=c['gamma_q'], epsilon=c['eps'],
                                        shared_policy=c['shared'], sr_by_elimination=True)
    mask = agent_mask(c, tabs)
    if mask is not None:
        agent.mask_actions, agent.action_mask = True, mask
    tr = pc.new_trace()
    for trials, steps, batch, no_replay in c['sessions']:
        agent.train(env, trials, steps, batch, no_replay, trace=tr)
    want = {'steps': np.array(tr['steps']), 'replay_start': tr['replay_start'],
            'replay_end': tr['replay_end'], 'last': np.array(tr['last']), 'Q': agent.Q,
            'T': mem.T, 'rewards': mem.rewards, 'states': mem.states, 'terminals': mem.terminals,
            'index': [env.rng.index, agent.policy.rng.index, mem.rng.index, mem.policy.rng.index]}
    return want, mem


# -- the device against it --------------------------------------------------------------------------
def run_case(c: dict) -> list:
    import pma_common as pc
    want, _ = run_reference(c)
    return _run_memory(c, want, pc) if c['kind'] == 'memory' else _run_agent(c, want, pc)


def _run_memory(c, want, pc) -> list:
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    n, pick = c['n'], c['pick']
    mem = PMAMemory(pc.sas_of(c['next']), EpsilonGreedy(c['eps']), gamma=c['gamma'],
                    gamma_q=c['gamma_q'], wide=c['wide'])
    mem.bind(n, seed=SEED, instance_base=c['base'])
    got = pc.ScriptMemory(
        mem, c['mask'], pick=None if n == 1 else pick,
        index=lambda m: (int(m.counter[pick].item()), int(m.policy.counter[pick].item()))).run(c['ops'])
    try:
        pc.assert_same_record(got, want, keys=pc.RECORD_KEYS + ('SR', 'need'))
    except AssertionError as err:
        return [str(err)[:300]]
    return []


def _run_agent(c, want, pc) -> list:
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    n, pick = c['n'], c['pick']
    world = agent_world(c)
    tabs = world.compact()
    env = Gridworld(world, n_envs=n, seed=SEED, instance_base=c['base'])
    pol = EpsilonGreedy(c['eps'])
    mem = PMAMemory(pc.sas_of(tabs['next']), pol if c['shared'] else EpsilonGreedy(c['eps']),
                    gamma_q=c['gamma_q'], wide=c['wide'])
    mine = (lambda x: x) if n == 1 else (lambda x: x[pick])
    seen = []
    agent = PMA(env.observation_space, env.action_space, pol, mem, custom_callbacks={
        'on_replay_end': [lambda logs: seen.append(pc.rows_of(mine(logs['replay'])))]})
    mask = agent_mask(c, tabs)
    if mask is not None:
        agent.mask_actions, agent.action_mask = True, mask
    agent.track_instances = True
    for trials, steps, batch, no_replay in c['sessions']:
        agent.train(env, trials, steps, batch, no_replay)
    bad = []

    def cmp(name, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        if got.shape != ref.shape or not np.array_equal(got, ref):
            bad.append(name)

    table = (lambda a: np.asarray(a)) if n == 1 else (lambda a: np.asarray(a)[pick])
    total = len(want['steps'])
    cmp('lat_trace', agent.monitors.lat_trace.cpu().numpy()[pick][:total], want['steps'])
    cmp('replays', len(seen), len(want['replay_start']) + len(want['replay_end']))
    for k, (a, b) in enumerate(zip(seen[0::2], want['replay_start'])):
        cmp('replay at the start of replayed trial %d' % k, a, b)
    for k, (a, b) in enumerate(zip(seen[1::2], want['replay_end'])):
        cmp('replay at the end of replayed trial %d' % k, a, b)
    cmp('Q', agent.Q if n == 1 else agent.Q.cpu().numpy()[pick], want['Q'])
    for name in ('T', 'rewards', 'states', 'terminals'):
        cmp(name, table(getattr(mem, name)), want[name])
    cmp('index', [int(env.env_ctr[pick].item()), int(agent.policy.counter[pick].item()),
                  int(mem.counter[pick].item()), int(mem.policy.counter[pick].item())], want['index'])
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
