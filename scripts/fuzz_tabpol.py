"""Randomised parity sweep for the tabular policy kernel (csrc/tabular_policy.hip): QAgent and DynaQ
with a Softmax, an ExclusiveEpsilonGreedy or a RandomDiscrete policy on random gridworlds (1 x 2 to
10 x 10 with the ingredients of scripts/fuzz_vs_oracle.py, and 31 x 33 / 32 x 32: 1 023 and 1 024
states), random graphs of 1..40 nodes with 1..8 actions (the generator of scripts/fuzz_topology.py)
and stacks of up to three gridworlds, through scripts of two to five operations on the SAME agent:

    train           agent.train with the case's policy
    train_budget    the same session cut into launches of 1 or 7 steps per instance
    test_default    agent.test with policy_test left at its default (the training policy's object)
    test_second     agent.test with a second Softmax / Exclusive / Random object as policy_test
    test_eps        agent.test with an EpsilonGreedy as policy_test (the other kernels)
    edit            rewards, terminals and the start list of env.world edited between two sessions
    train_eps       agent.train under an EpsilonGreedy, on the other kernels (k_tab_pwg and its
                    relatives read the model digest the policy kernel wrote)

    python scripts/fuzz_tabpol.py [first_seed] [count]

``train_eps`` is driven by ASSIGNING ``agent.policy`` for the session and putting the case's policy
back after it (``train()`` then sizes QAgent's log as it always does; ``Agent._session(pol=...)``
would run the same launches).  Every policy object keeps its own counter on its stream: the
training policies STREAM_POLICY, each ``policy_test`` of its own STREAM_POLICY_TEST, all from 0.

The checker is the restatement of tests/tabpol_common.py (``Restated`` over oracle/ref_loop.py on
``TapeRNG`` tapes), pinned to the real reference by tests/golden/tabpol_sweep_traces.npz.  It is
Python, so at most ten instances of a case are restated (``restated_instances``); after EVERY
operation their Q, model tables / log, counters, carried state and per-trial latencies are compared
with ``np.array_equal``, and for all instances on the device: a test session leaves Q, model, log,
memory counters and ``batches_done`` as they were, Dyna-Q's digest equals
``cobel_model_index_build`` of its model, ``env_steps()`` equals the latencies' sum.

A Softmax selection of the device may differ from NumPy's in the last bits (tabpol_common.py): a
case whose restatement meets a draw closer than ``SWEEP_MARGIN`` to an edge of its CDF is left out
and listed in ``REFUSED``, never silently.  ``run_reference(case)`` needs no GPU.  Reads only
oracle/ and tests/ (and, for its graphs, the generator of scripts/fuzz_topology.py).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'cobel-rl_amd'), ROOT,
           os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tabpol_common as tc  # noqa: E402
from fuzz_topology import draw_graph  # noqa: E402

SEED = tc.SEED
REFUSED: list = []      # seeds left out: a draw within SWEEP_MARGIN of an edge of its CDF
MAX_RESTATED = 10
ALPHAS = [0.99, 0.9, 0.5, 0.1, 1.0]          # scripts/fuzz_vs_oracle.py's sets
GAMMAS = [0.99, 0.9, 0.5, 0.0, 1.0]
REWARDS = [1.0, 1.0, 0.5, -1.0, 2.5, 0.0, -0.25, 1e-3]
BETAS = [0.05, 0.5, 2.0, 20.0, 1e3, 1e4]
EPSILONS = [0.0, 0.1, 0.3, 1.0]
SESSIONS = ('train', 'train_budget', 'test_default', 'test_second', 'test_eps', 'train_eps')
OPS = SESSIONS + ('edit',)


def _policy(r):
    kind = [tc.SOFTMAX, tc.EXCLUSIVE, tc.RANDOM][int(r.integers(0, 3))]
    par = None
    if kind == tc.SOFTMAX:
        par = float(r.choice(BETAS))
    elif kind == tc.EXCLUSIVE:
        par = float(r.choice(EPSILONS))
    return kind, par


def _grid(r, H, W, plain=False) -> dict:
    """The ingredients of fuzz_vs_oracle.draw_case for an H x W gridworld (``plain``: the two worlds
    at the top of the range get terminals, rewards and a few walls only)."""
    S = H * W
    terminals = sorted(set(int(x) for x in r.integers(0, S, int(r.integers(0, 4)))))
    rew_states = sorted(set(int(x) for x in r.integers(0, S, int(r.choice([0, 1, 1, 2, 2, 3, 6])))))
    for t in terminals:
        if r.random() < 0.7 and t not in rew_states:
            rew_states.append(t)
    vals = r.choice(REWARDS, len(rew_states))
    rewards = [[int(s), float(v)] for s, v in zip(rew_states, vals)]
    invalid = sorted(set(int(x) for x in r.integers(0, S, int(r.integers(0, max(1, S // 6)))))
                     - set(terminals))
    trans = []
    for _ in range(int(r.integers(0, 6))):
        a = int(r.integers(0, S))
        b = a + int(r.choice([-1, 1, -W, W]))
        if 0 <= b < S:
            trans.append((a, b))
    starts = None
    if r.random() < 0.4:
        starts = sorted(set(int(x) for x in r.integers(0, S, int(r.integers(1, 6))))
                        - set(terminals) - set(invalid)) or None
    wind_seed = int(r.integers(0, 1 << 31)) if r.random() < 0.15 else None
    if plain:
        invalid, trans, wind_seed = invalid[:8], [], None
    if len(set(terminals) | set(invalid)) >= S:      # (a world needs a state to start in)
        terminals, invalid = [], []
    return dict(H=H, W=W, terminals=terminals, rewards=rewards, invalid=invalid, trans=trans,
                starts=starts, wind_seed=wind_seed)


def draw_case(seed: int) -> dict:
    r = np.random.default_rng(7_000_003 * seed + 29)
    shape = r.random()
    c = dict(seed=seed)
    if shape < 0.6:
        c.update(world='grid', A=4, grid=_grid(r, int(r.integers(1, 11)), int(r.integers(2, 11))))
    elif shape < 0.9:
        S, A = int(r.integers(1, 41)), int(r.integers(1, 9))
        nbr, terminal, reward, starts = draw_graph(r, S, A)
        c.update(world='graph', A=A, graph=dict(
            S=S, nbr=nbr.tolist(), terminal=[bool(t) for t in terminal],
            reward=[float(x) for x in reward], starts=starts))
    else:
        H, W = [(31, 33), (32, 32)][int(r.integers(0, 2))]
        c.update(world='grid', A=4, grid=_grid(r, H, W, plain=True))
    c['S'] = c['grid']['H'] * c['grid']['W'] if c['world'] == 'grid' else c['graph']['S']
    big = c['S'] > 100
    # (a Topology is one graph, and DynaQ takes Discrete observations: gridworlds)
    c['extra_worlds'] = int(r.choice([0, 0, 1, 2])) if c['world'] == 'grid' else 0
    c['world_seed'] = int(r.integers(0, 1 << 31))
    c['base'] = int(r.choice([0, 5, 1 << 20]))
    c['agent'] = 'q' if c['world'] == 'graph' else ['dynaq', 'q'][int(r.integers(0, 2))]
    c['policy'] = _policy(r)
    c['alpha'], c['gamma'] = float(r.choice(ALPHAS)), float(r.choice(GAMMAS))
    c['n'] = int(r.choice([1, 2, 3, 7, 8, 9, 63, 64, 65, 130, 257]))
    c['batch'] = int(r.choice([0, 1, 2, 5, 8, 31, 32, 61, 62]))
    c['no_replay'] = bool(c['agent'] == 'dynaq' and r.random() < 0.1)
    c['mask_seed'] = int(r.integers(0, 1 << 31)) if r.random() < 0.25 else None
    # per-instance columns: policy parameter, learning rate, discount
    c['psets'] = None
    if c['n'] > 1 and r.random() < 0.3:
        n, kind = c['n'], c['policy'][0]
        if r.random() < 0.5:      # 2..4 combinations shared among the instances
            k = int(r.integers(2, 5))
            which = r.integers(0, k, n)
            par = {tc.SOFTMAX: r.choice(BETAS, k), tc.EXCLUSIVE: r.choice(EPSILONS, k),
                   tc.RANDOM: np.zeros(k)}[kind]
            al, ga = r.choice(ALPHAS, k), r.choice(GAMMAS, k)
            c['psets'] = dict(shared=k, par=[float(par[j]) for j in which],
                              alpha=[float(al[j]) for j in which], gamma=[float(ga[j]) for j in which])
        else:                     # every instance a combination of its own
            par = {tc.SOFTMAX: 0.05 + 20.0 * r.random(n), tc.EXCLUSIVE: r.random(n),
                   tc.RANDOM: np.zeros(n)}[kind]
            c['psets'] = dict(shared=0, par=[float(x) for x in par],
                              alpha=[float(x) for x in 0.1 + 0.9 * r.random(n)],
                              gamma=[float(x) for x in r.random(n)])
    c['second'] = _policy(r)                      # the second policy object of test_second
    c['eps_test'] = float(r.choice([0.0, 0.2]))   # the EpsilonGreedy of test_eps
    c['eps_train'] = float(r.choice([0.1, 0.3, 1.0, 0.0]))
    ops = []
    for k in range(int(r.integers(2, 6))):
        kind = OPS[int(r.integers(0, len(OPS)))]
        if k == 0 and r.random() < 0.8:           # (mostly something is learnt first)
            kind = SESSIONS[int(r.integers(0, 2))]
        op = dict(op=kind)
        if kind == 'edit':
            op['edit_seed'] = int(r.integers(0, 1 << 31))
        else:
            op['trials'] = int(r.integers(1, 4))
            op['steps'] = int(r.integers(1, 9 if big else 25))
            if kind == 'train_budget':
                op['budget'] = int(r.choice([1, 7]))
        ops.append(op)
    c['ops'] = ops
    return c


def describe(c: dict) -> str:
    w = '%(H)dx%(W)d' % c['grid'] if c['world'] == 'grid' else 'graph S=%d' % c['S']
    ps = c['psets']
    return ('seed %d %s %s A=%d worlds=1+%d n=%d base=%d %s B=%d a=%g g=%g%s%s%s second=%s ops=%s'
            % (c['seed'], c['agent'], w, c['A'], c['extra_worlds'], c['n'], c['base'], c['policy'],
               c['batch'], c['alpha'], c['gamma'], ' no_replay' if c['no_replay'] else '',
               ' masked' if c['mask_seed'] is not None else '',
               '' if ps is None else (' sets=%s' % (ps['shared'] or 'distinct')), c['second'],
               [' '.join('%s' % v for v in o.values()) for o in c['ops']]))


# -- the worlds of a case (no GPU) --------------------------------------------------------------------
def grid_worlds(c: dict, make_gridworld=None) -> list:
    """The ``World`` dictionaries of a gridworld case: the drawn one, then the extra worlds of the
    same shape (other walls, goals and rewards); by the product's builder or the one handed in."""
    if make_gridworld is None:
        from cobel_amd.misc.gridworld_tools import make_gridworld
    g = c['grid']
    H, W, S = g['H'], g['W'], c['S']
    wind = None if g['wind_seed'] is None else np.random.default_rng(g['wind_seed']).integers(-1, 2, (S, 2))
    world = make_gridworld(H, W, terminals=g['terminals'],
                           rewards=np.array(g['rewards'], dtype=np.float64).reshape(-1, 2),
                           goals=g['terminals'], starting_states=g['starts'],
                           invalid_states=g['invalid'], invalid_transitions=g['trans'], wind=wind)
    if len(world['starting_states']) == 0:
        world = make_gridworld(H, W, rewards=np.array(g['rewards'], dtype=np.float64).reshape(-1, 2))
    worlds = [world]
    wr = np.random.default_rng(c['world_seed'])
    for _ in range(c['extra_worlds']):
        inv = sorted(set(int(x) for x in wr.integers(0, S, int(wr.integers(0, max(1, S // 5))))))[:8]
        term = sorted(set(int(x) for x in wr.integers(0, S, int(wr.integers(0, 3)))) - set(inv))
        rw = np.array([[int(wr.integers(0, S)), float(wr.choice([1.0, -0.5, 2.0]))]
                       for _ in range(int(wr.integers(0, 3)))], dtype=np.float64).reshape(-1, 2)
        w2 = make_gridworld(H, W, terminals=term, rewards=rw, goals=term, invalid_states=inv)
        if len(w2['starting_states']) == 0:
            w2 = make_gridworld(H, W, rewards=rw)
        worlds.append(w2)
    return worlds


def graph_nodes(c: dict):
    g = c['graph']
    nodes = {}
    for i in range(g['S']):
        nodes[str(i)] = {'id': str(i), 'pose': np.array([float(i % 7), float(i // 7), 0.0, 0.0, 0.0, 0.0]),
                         'neighbors': [str(int(j)) for j in g['nbr'][i]],
                         'reward': float(g['reward'][i]), 'terminal': bool(g['terminal'][i])}
    starts = None if g['starts'] is None else [str(s) for s in g['starts']]
    if starts is None:
        starts = [k for k, nd in nodes.items() if not nd['terminal']]
    return nodes, starts


def case_tables(c: dict) -> list:
    """The compact tables of the case's worlds, in world order."""
    if c['world'] == 'graph':
        return [tc.node_tables(*graph_nodes(c))]
    return [tc.world_tables(w) for w in grid_worlds(c)]


def case_mask(c: dict):
    if c['mask_seed'] is None:
        return None
    S, A = c['S'], c['A']
    m = np.random.default_rng(c['mask_seed']).random((S, A)) < 0.7
    m[np.arange(S), np.random.default_rng(c['mask_seed'] + 1).integers(0, A, S)] = True
    return m


def edited_tables(tabs: dict, edit_seed: int) -> dict:
    """Tables after a world edit: one to three rewards rewritten, one terminal flag flipped, a new
    start list of one to four non-terminal states the old world could start in or pass through."""
    r = np.random.default_rng(edit_seed)
    S = len(tabs['reward'])
    reward, terminal = np.array(tabs['reward'], dtype=np.float64), np.array(tabs['terminal'], dtype=np.uint8)
    for s in r.integers(0, S, int(r.integers(1, 4))):
        reward[int(s)] = float(r.choice(REWARDS))
    flip = int(r.integers(0, S))
    terminal[flip] ^= 1
    nxt = np.asarray(tabs['next'])
    # (states something leads to, and the old starts: never the inside of a wall)
    live = np.union1d(np.unique(nxt[np.asarray(tabs['starts'], dtype=np.int64)]),
                      np.asarray(tabs['starts'], dtype=np.int64))
    free = [int(s) for s in live if not terminal[int(s)]]
    if not free:
        terminal[flip] ^= 1
        free = [int(s) for s in live if not terminal[int(s)]]
    starts = sorted(set(int(x) for x in r.choice(free, int(r.integers(1, 5)))))
    return dict(next=nxt, reward=reward, terminal=terminal, starts=np.array(starts, dtype=np.uint16))


def columns(c: dict, i=None):
    """(policy parameter, alpha, gamma): of instance i, or the scalars / per-instance arrays the
    device classes take."""
    ps, (kind, par) = c['psets'], c['policy']
    if ps is None:
        return par, c['alpha'], c['gamma']
    if i is None:
        return (None if kind == tc.RANDOM else np.array(ps['par'])), np.array(ps['alpha']), np.array(ps['gamma'])
    return (None if kind == tc.RANDOM else ps['par'][i]), ps['alpha'][i], ps['gamma'][i]


def restated_instances(c: dict, ipw: int = 8) -> list:
    """At most ``MAX_RESTATED`` instances: 0, 1, n - 1, the first instance of each world, then the
    instances on either side of the multiples of ``ipw`` (instances per workgroup; without a device
    to ask, 8 — a multiple of every count the planner hands out), the outermost multiples first."""
    n, n_worlds = c['n'], 1 + c['extra_worlds']
    want = [0, 1, n - 1]
    want += [(w - c['base']) % n_worlds for w in range(n_worlds)]
    mults = list(range(ipw, n, ipw))
    order = []
    while mults:
        order.append(mults.pop(0))
        if mults:
            order.append(mults.pop())
    for m in order:
        want += [m - 1, m]
    out = []
    for i in want:
        if 0 <= i < n and i not in out and len(out) < MAX_RESTATED:
            out.append(i)
    return out


class Reference:
    """The restated instances of a case, stepped one operation at a time."""

    def __init__(self, c: dict, instances):
        self.c, self.tabs, self.mask = c, case_tables(c), case_mask(c)
        self.refs, self.second, self.eps_test, self.eps_train = {}, {}, {}, {}
        for i in instances:
            g = c['base'] + i
            par, alpha, gamma = columns(c, i)
            self.refs[i] = tc.Restated(self.tabs[g % len(self.tabs)], c['agent'], (c['policy'][0], par),
                                       g, alpha=alpha, gamma=gamma, mask=self.mask)

    def _object(self, store, i, spec, stream):
        if i not in store:
            store[i] = self.refs[i].policy_object(spec, stream)
        return store[i]

    def apply(self, op: dict) -> None:
        from oracle.philox import STREAM_AUX, STREAM_POLICY
        c = self.c
        if op['op'] == 'edit':
            self.tabs[0] = edited_tables(self.tabs[0], op['edit_seed'])
            for i, r in self.refs.items():
                if (c['base'] + i) % len(self.tabs) == 0:
                    r.edit_world(self.tabs[0])
            return
        for i, r in self.refs.items():
            how = (op['trials'], op['steps'], c['batch'])
            if op['op'] in ('train', 'train_budget'):
                r.session(r.pol, *how, True, c['no_replay'])
            elif op['op'] == 'train_eps':
                pol = self._object(self.eps_train, i, ('eps', c['eps_train']), STREAM_POLICY)
                r.session(pol, *how, True, c['no_replay'])
            elif op['op'] == 'test_default':
                r.session(r.pol, *how, False)
            elif op['op'] == 'test_second':
                r.session(self._object(self.second, i, c['second'], STREAM_AUX), *how, False)
            else:
                r.session(self._object(self.eps_test, i, ('eps', c['eps_test']), STREAM_AUX), *how, False)

    def snapshot(self, i) -> dict:
        r = self.refs[i]
        d = r.record()
        for name, store in (('second', self.second), ('eps_test', self.eps_test), ('eps_train', self.eps_train)):
            d['ctr_' + name] = np.int64(store[i].rng.index if i in store else 0)
        return d

    def margin(self) -> float:
        return min(r.margin() for r in self.refs.values())


def run_reference(c: dict, ipw: int = 8, instances=None) -> dict:
    """The restatement alone: {instance: [snapshot after every operation]} plus ``'margin'``, the
    least distance of a draw from an edge of its CDF, and ``'underflow'``, whether a Softmax
    probability of an action on offer came out as exact zero."""
    inst = restated_instances(c, ipw) if instances is None else list(instances)
    with np.errstate(invalid='ignore', divide='ignore'):    # (Exclusive, epsilon 1, all tied: 0 / 0)
        ref = Reference(c, inst)
        out = {i: [] for i in inst}
        for op in c['ops']:
            ref.apply(op)
            for i in inst:
                out[i].append(ref.snapshot(i))
    out['margin'] = ref.margin()
    out['underflow'] = any(getattr(p, 'underflowed', False) for r in ref.refs.values() for p in r.policies)
    return out


# -- the device -----------------------------------------------------------------------------------------
def device_case(c: dict):
    """(environment, agent, the policy objects by role) of a case on the device."""
    from cobel_amd.interface import Gridworld, Topology
    if c['world'] == 'graph':
        nodes, starts = graph_nodes(c)
        env = Topology(nodes, starts, n_envs=c['n'], seed=SEED, instance_base=c['base'])
    else:
        worlds = grid_worlds(c)
        env = Gridworld(worlds if len(worlds) > 1 else worlds[0], n_envs=c['n'], seed=SEED,
                        instance_base=c['base'])
    assert int(env.action_space.n) == c['A']
    par, alpha, gamma = columns(c)
    ag = tc.device_agent(env, c['agent'], (c['policy'][0], par), alpha=alpha, gamma=gamma,
                         mask=case_mask(c))
    pols = dict(main=ag.policy, second=tc.device_policy(c['second'], c['A']),
                eps_test=tc.device_policy(('eps', c['eps_test']), c['A']),
                eps_train=tc.device_policy(('eps', c['eps_train']), c['A']))
    return env, ag, pols


def budgeted_train(ag, env, c: dict, trials: int, steps: int, budget: int) -> None:
    """agent.train(...) as launches of ``budget`` steps per instance: the steps of Agent._session
    written out (the loop of fuzz_vs_oracle.session on the policy path)."""
    from cobel_amd import _lib
    ag._bind(env)
    if c['agent'] == 'q':
        used = int(ag.inst[:, _lib.I_LOG_LEN].max().item())
        ag.reserve_replay(used + trials * steps)
        ag._log_now = True
    extra = _lib.F_NO_REPLAY if c['no_replay'] else 0
    pol, flags, first = ag._session_begin(env, trials, True, extra)
    target = first + trials
    for _ in range(trials * steps + 1):
        ag._launch(env, pol, flags, target, steps, budget, c['batch'])
        if int(ag.inst[:, _lib.I_TRIAL].min().item()) >= target:
            break
    else:
        raise AssertionError('budgeted launches did not finish the session')
    ag.current_trial = target
    ag._session_end(pol, env)


def device_edit(env, c: dict, tabs: dict) -> None:
    """The edit as a user makes it: rewards and terminals in place, the start list replaced."""
    if c['world'] == 'graph':
        for i, k in enumerate(env.ids):
            env.nodes[k]['reward'] = float(tabs['reward'][i])
            env.nodes[k]['terminal'] = bool(tabs['terminal'][i])
        env.starting_nodes = [env.ids[int(j)] for j in tabs['starts']]
        return
    env.world['rewards'][:] = tabs['reward']
    env.world['terminals'][:] = tabs['terminal']
    env.world['starting_states'] = np.array(tabs['starts'], dtype=int)


def device_apply(env, ag, pols, c: dict, op: dict) -> None:
    how = (op['trials'], op['steps'])
    train = (lambda: ag.train(env, *how, c['batch'], c['no_replay'])) if c['agent'] == 'dynaq' else \
        (lambda: ag.train(env, *how, c['batch']))
    if op['op'] == 'train':
        train()
    elif op['op'] == 'train_budget':
        budgeted_train(ag, env, c, *how, op['budget'])
    elif op['op'] == 'train_eps':
        ag.policy = pols['eps_train']
        try:
            train()
        finally:
            ag.policy = pols['main']
    else:
        ag.policy_test = pols[{'test_default': 'main', 'test_second': 'second', 'test_eps': 'eps_test'}[op['op']]]
        ag.test(env, *how)


def whole_state(ag) -> dict:
    """What a test session may not touch, for all instances."""
    from cobel_amd import _lib
    d = dict(Q=ag._q.clone(), batches_done=ag.batches_done.clone(),
             ctr_memory=ag.inst[:, _lib.I_CTR_MEMORY].clone(), log_len=ag.inst[:, _lib.I_LOG_LEN].clone())
    if c_is_dynaq(ag):
        d.update(model=ag.M.table.clone(), index=ag.M.index.clone(), M_counter=ag.M.counter.clone())
    elif ag._log is not None:
        d['log'] = ag._log.clone()
    return d


def c_is_dynaq(ag) -> bool:
    from cobel_amd import _lib
    return ag.agent_kind == _lib.AGENT_DYNAQ


def trial_rewards_f32(trace: dict) -> np.ndarray:
    """Per trial the float64 sum, in step order, of the rewards as the device's world record holds
    them (float32): what a kernel adds up for RewardMonitor."""
    r = np.array([e[2] for e in trace['sarsn']], dtype=np.float64).astype(np.float32).astype(np.float64)
    out, at = [], 0
    for lat in trace['steps']:
        total = 0.0
        for x in r[at:at + lat + 1]:
            total += float(x)
        out.append(total)
        at += lat + 1
    return np.array(out)


def run_case(c: dict):
    """-> list of mismatches (empty: parity, or the case was left out: see ``REFUSED``)"""
    import torch
    from cobel_amd import _lib
    env, ag, pols = device_case(c)
    ag._bind(env)
    plan = ag.describe_launch(env, ag.policy, _lib.F_LEARN, 1, 1, 0, c['batch'])
    inst = restated_instances(c, plan['instances_per_workgroup'])
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = Reference(c, inst)
    bad = []
    trials_done = 0

    def cmp(what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append('%s: %s vs %s' % (what, got.ravel()[:6].tolist(), want.ravel()[:6].tolist())
                       if got.size <= 6 or got.shape != want.shape else
                       '%s: %d differ, first at %s' % (what, int((got != want).sum()),
                                                       np.argwhere(got != want)[0].tolist()))

    for k, op in enumerate(c['ops']):
        tag = 'op %d %s' % (k, op['op'])
        with np.errstate(invalid='ignore', divide='ignore'):
            ref.apply(op)
        if ref.margin() < tc.SWEEP_MARGIN:
            REFUSED.append(c['seed'])
            return []
        if op['op'] == 'edit':
            device_edit(env, c, ref.tabs[0])
            continue
        test = op['op'].startswith('test')
        before = whole_state(ag) if test else None
        others = {name: (None if p.counter is None else p.counter.clone()) for name, p in pols.items()}
        device_apply(env, ag, pols, c, op)
        torch.cuda.synchronize()
        trials_done += op['trials']
        acting = {'train': 'main', 'train_budget': 'main', 'train_eps': 'eps_train', 'test_default': 'main',
                  'test_second': 'second', 'test_eps': 'eps_test'}[op['op']]
        for name, ctr in others.items():      # a session advances the counter of its own policy only
            if name != acting and ctr is not None and not torch.equal(ctr, pols[name].counter):
                bad.append('%s: the counter of policy object %s moved' % (tag, name))
        if test:
            for name, was in before.items():
                now = whole_state(ag)[name]
                if not torch.equal(was, now):
                    bad.append('%s: a test session changed %s' % (tag, name))
        if c_is_dynaq(ag):
            fresh = torch.empty_like(ag.M.index)
            _lib.check(_lib.lib().cobel_model_index_build(_lib.ptr(ag.M.table), _lib.ptr(fresh), c['n'],
                                                          c['S'], None))
            torch.cuda.synchronize()
            if not torch.equal(fresh, ag.M.index):
                bad.append('%s: M.index is not the digest of M.table (%d entries)'
                           % (tag, int((fresh != ag.M.index).sum().item())))
        lat = ag.monitors.lat_trace.cpu().numpy()[:, :trials_done]
        raw = ag.inst.cpu().numpy()
        for i in inst:
            want = ref.snapshot(i)
            got = tc.device_tables(ag, i, c['A'])
            who = '%s instance %d ' % (tag, i)
            keys = ['Q', 'M_rewards', 'M_states', 'M_terminals', 'log', 'ctr_env']
            if c['batch'] > 0:    # (without a batch the reference still makes its empty draw; the kernels none)
                keys.append('ctr_memory')
            for key in keys:
                if key in want:
                    cmp(who + key, got[key], want[key])
            if 'log' in want:
                cmp(who + 'log length', int(raw[i, _lib.I_LOG_LEN]), len(want['log']))
            cmp(who + 'latencies', lat[i], want['steps'])
            cmp(who + 'carried state', int(raw[i, _lib.I_STATE]), int(want['env_state']))
            cmp(who + 'carried state (env)', int(env.state[i].item()), int(want['env_state']))
            for name, key in (('main', 'ctr_policy'), ('second', 'ctr_second'), ('eps_test', 'ctr_eps_test'),
                              ('eps_train', 'ctr_eps_train')):
                ctr = pols[name].counter
                cmp(who + key, 0 if ctr is None else int(ctr[i].item()), int(want[key]))
        if len(inst) == c['n']:      # the monitor sums over instances
            steps = np.array([ref.refs[i].trace['steps'] for i in inst])
            rew = np.array([trial_rewards_f32(ref.refs[i].trace) for i in inst])
            cmp(tag + ' lat_sum', ag.monitors.lat_sum.cpu().numpy()[:trials_done], steps.sum(axis=0))
            cmp(tag + ' lat_cnt', ag.monitors.lat_cnt.cpu().numpy()[:trials_done], np.full(trials_done, c['n']))
            # (the world record holds float32 rewards; float64 atomics in any order: the sums agree
            #  to rounding, not to the bit)
            if not np.allclose(ag.monitors.reward_sum.cpu().numpy()[:trials_done], rew.sum(axis=0),
                               rtol=1e-12, atol=1e-12):
                bad.append(tag + ' reward_sum')
        cmp(tag + ' env_steps', ag.env_steps(), int((lat.astype(np.int64) + 1).sum()))
        if pols['second'].stream is not None and pols['second'].stream != _lib.STREAM_POLICY_TEST:
            bad.append(tag + ': the second policy object is not on STREAM_POLICY_TEST')
        if pols['main'].stream not in (None, _lib.STREAM_POLICY):
            bad.append(tag + ': the training policy is not on STREAM_POLICY')
        if bad:
            break
    return bad


def main() -> int:
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    failed, t0 = [], time.time()
    for seed in range(first, first + count):
        c = draw_case(seed)
        try:
            bad = run_case(c)
        except Exception as e:      # a refused configuration is a finding too
            bad = ['%s: %s' % (type(e).__name__, str(e)[:300])]
        if bad:
            failed.append(seed)
            print('MISMATCH', bad[:4], describe(c), flush=True)
        if (seed - first) % 20 == 19:
            print('... %d cases, %d failing, %d left out, %.0f s'
                  % (seed - first + 1, len(failed), len(REFUSED), time.time() - t0), flush=True)
    print('cases %d, failing %d: %s; left out %d: %s; %.0f s'
          % (count, len(failed), failed, len(REFUSED), REFUSED, time.time() - t0))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
