"""Golden records that pin the extended restatement of tests/tabpol_common.py (test sessions of
QAgent, a tape per policy object, worlds edited between sessions) to the real reference.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_tabpol_sweep.py

Instance 0 of the seeds ``fuzz_tabpol_common.TABPOL_RECORDED`` of scripts/fuzz_tabpol.py is driven
through its script of operations with the reference's own classes on the build's Philox tapes (the
shim, the tapes and the two coercions are gen_tabpol.py's: float32 tables, float64 rows for
Softmax), then the test-session cases ``tabpol_common.TEST_CASES``.  How an operation reaches the
reference: ``train_budget`` is ``train`` (the reference has no launches to cut), ``train_eps`` and
the ``test_*`` operations assign ``agent.policy`` / ``agent.policy_test`` for their session, each
policy object on a tape of its own, an edit rewrites ``env.world`` / ``env.nodes`` in place.

Two things the reference cannot run are refused here, so the recorded seeds avoid them: a mask on a
QAgent (the reference's QAgent has none) and an ExclusiveEpsilonGreedy(1) on a row of nothing but
ties (Generator.choice raises).  As in gen_tabpol.py a record is kept only if every draw lies at
least ``MARGIN`` from every edge of its CDF.

Writes tabpol_sweep_traces.npz: per case what ``Restated.record`` returns — the steps of all
sessions, per trial the latencies, rewards and Q, the final Q, model / log, the counters of every
policy object, the carried state.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
import gen_tabpol as GT  # noqa: E402
from gen_golden import (SEED, STREAM_ENV, STREAM_MEMORY, STREAM_POLICY, DynaQ,  # noqa: E402
                        Gridworld, QAgent, TapeRNG, gt)

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
sys.path.insert(0, os.path.join(G.ROOT, 'scripts'))
import fuzz_tabpol as fz  # noqa: E402
import fuzz_tabpol_common as fa  # noqa: E402
import tabpol_common as tc  # noqa: E402

from cobel.interface import Topology  # noqa: E402
from oracle.philox import STREAM_AUX  # noqa: E402


class Driven:
    """One instance of the reference's agent and environment with recording callbacks."""

    def __init__(self, env, tabs, keys, agent, policy, g, test_policy=None, alpha=None, gamma=None,
                 mask=None):
        self.env, self.keys, self.g, self.kind = env, keys, g, agent
        self.A = tabs['next'].shape[1]
        self.margin = [float('inf')]
        self.pol = self.policy_object(policy, STREAM_POLICY)
        self.pol_test = None if test_policy is None else self.policy_object(test_policy, STREAM_AUX)
        self.mem = TapeRNG(SEED, g, STREAM_MEMORY)
        kw = {}
        if alpha is not None:
            kw['learning_rate'] = float(alpha)
        if gamma is not None:
            kw['gamma'] = float(gamma)
        if agent == 'dynaq':
            ag = DynaQ(env.observation_space, env.action_space, self.pol, self.pol_test, **kw)
            ag.M.rng = self.mem
            ag.Q = ag.Q.astype(np.float32)
            ag.M.rewards = ag.M.rewards.astype(np.float32)
            if mask is not None:
                ag.mask_actions, ag.action_mask = True, np.asarray(mask, dtype=bool)
            self.table = lambda: np.array(ag.Q, dtype=np.float32)
        else:
            assert mask is None, 'the reference\'s QAgent has no action mask: record another seed'
            ag = QAgent(env.observation_space, env.action_space, self.pol, self.pol_test, rng=self.mem, **kw)
            for k in keys:
                ag.Q[k] = np.zeros(self.A, dtype=np.float32)
            self.table = lambda: np.array([ag.Q[k] for k in keys], dtype=np.float32)
        self.ag = ag
        self.index = {k: i for i, k in enumerate(keys)}
        self.sarsn, self.tds, self.steps, self.rewards, self.q_trial = [], [], [], [], []
        first = lambda x: x if isinstance(x, tuple) else (int(x),)       # noqa: E731

        def on_step_end(logs):
            self.sarsn.append((self.index[first(logs['state'])], logs['action'], logs['reward'],
                               self.index[first(logs['next_state'])], logs['terminal']))
            td = logs.get('td', 0.0) if self.learning else 0.0
            self.tds.append(float(td) if np.ndim(td) == 0 else 0.0)

        def on_trial_end(logs):
            self.steps.append(logs['steps'])
            self.rewards.append(float(logs['trial_reward']))
            self.q_trial.append(self.table())

        ag.callbacks.custom_callbacks = {'on_step_end': [on_step_end], 'on_trial_end': [on_trial_end],
                                         'on_trial_begin': [], 'on_step_begin': []}
        self.learning = True
        self.first = first

    def policy_object(self, spec, stream):
        return GT.make_policy(spec, TapeRNG(SEED, self.g, stream), self.A, self.margin)

    def session(self, pol, trials, steps, batch, learn, no_replay=False):
        keep = self.ag.policy, self.ag.policy_test
        self.learning = learn
        if learn:
            self.ag.policy = pol
            if self.kind == 'dynaq':
                self.ag.train(self.env, trials, steps, batch, no_replay)
            else:
                self.ag.train(self.env, trials, steps, batch)
        else:
            self.ag.policy_test = pol
            self.ag.test(self.env, trials, steps)
        self.ag.policy, self.ag.policy_test = keep

    def record(self, state_index) -> dict:
        ag = self.ag
        assert self.table().dtype == np.float32
        a = np.array(self.sarsn, dtype=np.float64).reshape(-1, 5)
        d = dict(state=a[:, 0].astype(np.int16), action=a[:, 1].astype(np.int8), reward=a[:, 2],
                 next_state=a[:, 3].astype(np.int16), nonterminal=a[:, 4].astype(np.int8),
                 td=np.array(self.tds, dtype=np.float64), steps=np.array(self.steps, dtype=np.int32),
                 trial_reward=np.array(self.rewards, dtype=np.float64),
                 Q_trial=np.array(self.q_trial, dtype=np.float32), Q=self.table(),
                 ctr_env=np.int64(self.env.rng.index), ctr_policy=np.int64(self.pol.rng.index),
                 ctr_policy_test=np.int64(0 if self.pol_test is None else self.pol_test.rng.index),
                 ctr_memory=np.int64(self.mem.index), margin=np.float64(self.margin[0]),
                 env_state=np.int64(state_index))
        if self.kind == 'dynaq':
            assert ag.M.rewards.dtype == np.float32
            d.update(M_rewards=np.array(ag.M.rewards, dtype=np.float32),
                     M_states=ag.M.states.astype(np.int16), M_terminals=ag.M.terminals.astype(np.int8))
        else:
            d['log'] = tc.pack_log([(self.index[self.first(e['state'])], e['action'], e['reward'],
                                     self.index[self.first(e['next_state'])], e['terminal'])
                                    for e in ag.M], self.A)
        return d


def run_seed(seed) -> dict:
    c = fz.draw_case(seed)
    g = c['base']                        # instance 0
    rng = TapeRNG(SEED, g, STREAM_ENV)
    if c['world'] == 'graph':
        nodes, starts = fz.graph_nodes(c)
        for nd in nodes.values():
            nd['pose'] = tuple(float(x) for x in nd['pose'])
        env = Topology(nodes, starts, None, rng=rng)
        tabs = tc.node_tables(nodes, starts)
        ids = list(nodes.keys())
        keys = [tuple(np.array(nodes[k]['pose']).flatten()) for k in ids]
        which = 0
    else:
        worlds = fz.grid_worlds(c, gt.make_gridworld)
        which = g % len(worlds)
        env = Gridworld(worlds[which], rng=rng)
        tabs = tc.world_tables(worlds[which])
        keys = [(s,) for s in range(c['S'])]
    # (the builders of the reference and of the project give the same tables)
    mine = fz.case_tables(c)[which]
    assert all(np.array_equal(tabs[k], mine[k]) for k in tabs), 'seed %d: the builders differ' % seed
    par, alpha, gamma = fz.columns(c, 0)
    d = Driven(env, tabs, keys, c['agent'], (c['policy'][0], par), g, alpha=alpha, gamma=gamma,
               mask=fz.case_mask(c))
    objects = {}
    first_world = fz.case_tables(c)[0]

    def obj(name, spec, stream):
        if name not in objects:
            objects[name] = d.policy_object(spec, stream)
        return objects[name]

    for op in c['ops']:
        if op['op'] == 'edit':
            tabs = first_world = fz.edited_tables(first_world, op['edit_seed'])
            if which != 0:
                continue                 # (env.world is the first world: instance 0 lives elsewhere)
            if c['world'] == 'graph':
                for i, k in enumerate(ids):
                    env.nodes[k]['reward'] = float(tabs['reward'][i])
                    env.nodes[k]['terminal'] = bool(tabs['terminal'][i])
                env.starting_nodes = [ids[int(j)] for j in tabs['starts']]
            else:
                env.world['rewards'][:] = tabs['reward']
                env.world['terminals'][:] = tabs['terminal']
                env.world['starting_states'] = np.array(tabs['starts'], dtype=int)
            continue
        how = (op['trials'], op['steps'], c['batch'])
        if op['op'] in ('train', 'train_budget'):
            d.session(d.pol, *how, True, c['no_replay'])
        elif op['op'] == 'train_eps':
            d.session(obj('eps_train', ('eps', c['eps_train']), STREAM_POLICY), *how, True, c['no_replay'])
        elif op['op'] == 'test_default':
            d.session(d.pol, *how, False)
        elif op['op'] == 'test_second':
            d.session(obj('second', c['second'], STREAM_AUX), *how, False)
        else:
            d.session(obj('eps_test', ('eps', c['eps_test']), STREAM_AUX), *how, False)
    state = ids.index(env.current_node) if c['world'] == 'graph' else int(env.current_state)
    out = d.record(state)
    for name in ('second', 'eps_test', 'eps_train'):
        out['ctr_' + name] = np.int64(objects[name].rng.index if name in objects else 0)
    return out


def run_test_case(name) -> dict:
    c = tc.session_case(name)
    world = tc.grid4(gt)
    env = Gridworld(world, rng=TapeRNG(SEED, c['inst'], STREAM_ENV))
    tabs = tc.world_tables(world)
    d = Driven(env, tabs, [(s,) for s in range(int(world['states']))], c['agent'], c['policy'],
               c['inst'], test_policy=c['test'])
    d.session(d.pol, tc.TRIALS, tc.STEPS, tc.TEST_BATCH, True)
    n_train = len(d.sarsn)
    d.learning = False
    d.ag.test(env, tc.TEST_TRIALS, tc.TEST_STEPS)     # (policy_test as the constructor left it)
    out = d.record(int(env.current_state))
    out['n_train_steps'] = np.int64(n_train)
    return out


def main() -> None:
    out = {}
    todo = [('seed%d' % s, (lambda s=s: run_seed(s))) for s in fa.TABPOL_RECORDED]
    todo += [(name, (lambda name=name: run_test_case(name))) for name in tc.TEST_CASES]
    for name, run in todo:
        with np.errstate(invalid='raise'):      # (0 / 0 in a CDF: Generator.choice would have raised)
            d = run()
        assert d['margin'] > tc.MARGIN, '%s: a draw within 1e-9 of an edge of its CDF (%g): take ' \
                                        'another seed or instance number' % (name, d['margin'])
        print('%-22s steps %4d margin %.3g' % (name, len(d['state']), d['margin']))
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v
    path = G._out('tabpol_sweep_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
