"""Golden trajectories of test sessions, recorded from the real reference.

The reference's ``DynaQ.test`` / ``QAgent.test`` (agent/dyna_q.py:217-273, agent/q.py:230-287) run
with its own ``TrajectoryMonitor`` (monitor/behavior.py:304-385) under ``on_step_end`` and with
``agent.Q`` set to planted float32 tables: all zeros (every selection a four-way tie), a plateau
table with two-way ties, and a table the reference trained for 20 trials.  Worlds: the 5x5 open
field, the 8x8 world with walls under ``mask_actions``, ``linear_track(4, 1)``.  Every case starts
from fresh streams (the constructor's start draw, then the session), so a test replays it from the
planted table alone.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_rollout.py

Reuses the shim and the tape generators of gen_golden.py; the cases and tables are
tests/rollout_common.py's.  Writes rollout_traces.npz: per case the table, the start states, the
per-step states and actions (padded -1 / 255), ``logs['steps']`` and the monitor's position lists
(concatenated; trial t holds ``steps[t] + 1`` rows).
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
import rollout_common as rc  # noqa: E402

from cobel.interface import Topology  # noqa: E402
from cobel.misc import topology_tools as tt  # noqa: E402
from cobel.monitor import TrajectoryMonitor  # noqa: E402
from oracle.philox import STREAM_AUX  # noqa: E402  (the stream of a policy_test of its own)

assert SEED == rc.SEED


def build(c):
    """Environment, state-key table and compact tables of a case, on fresh tapes."""
    rng = TapeRNG(SEED, c['inst'], STREAM_ENV, double_sub=1)
    if c['world'] == 'track4':
        nodes, starts = tt.linear_track(4, 1)
        env = Topology(nodes, starts, None, rng=rng)
        tabs = rc.node_tables(nodes, starts)
        keys = [tuple(np.array(nodes[k]['pose']).flatten()) for k in nodes]
    else:
        world = rc.grid_world(gt, c['world'])
        env = Gridworld(world, rng=rng)
        tabs = rc.world_tables(world)
        keys = [(s,) for s in range(int(world['states']))]
    return env, keys, tabs


def agent_for(c, env, keys, tabs, q, test_run: bool):
    """The reference's agent with ``q`` planted (float32 rows)."""
    pol = EpsilonGreedy(c['eps'], rng=TapeRNG(SEED, c['inst'], STREAM_POLICY))
    pol_test = None
    if test_run and c['test_policy']:
        pol_test = EpsilonGreedy(c['eps'], rng=TapeRNG(SEED, c['inst'], STREAM_AUX))
    if c['agent'] == 'dynaq':
        ag = DynaQ(env.observation_space, env.action_space, pol, pol_test)
        ag.M.rng = TapeRNG(SEED, c['inst'], STREAM_MEMORY)
        ag.M.rewards = ag.M.rewards.astype(np.float32)
        ag.Q = np.array(q, dtype=np.float32)
        if c['mask']:
            ag.mask_actions, ag.action_mask = True, rc.bump_mask(tabs['next'])
    else:
        ag = QAgent(env.observation_space, env.action_space, pol, pol_test,
                    rng=TapeRNG(SEED, c['inst'], STREAM_MEMORY))
        for k, row in zip(keys, q):
            ag.Q[k] = np.array(row, dtype=np.float32)
    return ag


def trained_table(c) -> np.ndarray:
    """The table after TRAIN_TRIALS trials of the reference's train() on float32 rows."""
    env, keys, tabs = build(c)
    n_states, n_actions = tabs['next'].shape
    ag = agent_for(c, env, keys, tabs, np.zeros((n_states, n_actions), dtype=np.float32), False)
    ag.callbacks.custom_callbacks = {k: [] for k in ('on_trial_begin', 'on_trial_end',
                                                     'on_step_begin', 'on_step_end')}
    ag.train(env, rc.TRAIN_TRIALS, c['steps'], 8)
    if c['agent'] == 'dynaq':
        return np.array(ag.Q, dtype=np.float32)
    return np.array([ag.Q[k] for k in keys], dtype=np.float32)


def run_case(name) -> dict:
    c = rc.case(name)
    env, keys, tabs = build(c)
    n_states, n_actions = tabs['next'].shape
    q = rc.planted_table(c['table'], n_states, n_actions)
    if q is None:
        q = trained_table(c)
    assert q.dtype == np.float32
    ag = agent_for(c, env, keys, tabs, q, True)
    index = {k: i for i, k in enumerate(keys)}
    first = lambda x: x if isinstance(x, tuple) else (int(x),)       # noqa: E731
    sarsn, steps_log = [], []
    monitor = TrajectoryMonitor(c['trials'], env)
    ag.callbacks.custom_callbacks = {
        'on_step_end': [monitor.update,
                        lambda logs: sarsn.append((index[first(logs['state'])], logs['action'], 0.0,
                                                   index[first(logs['next_state'])], 0))],
        'on_trial_end': [lambda logs: steps_log.append(logs['steps'])],
        'on_trial_begin': [], 'on_step_begin': []}
    ag.test(env, c['trials'], c['steps'])
    d = rc.pack_session(sarsn, steps_log, c['trials'], c['steps'])
    trace = monitor.get_trace()
    assert [len(t) for t in trace] == [int(n) for n in d['length']]
    d['steps_log'] = np.array(steps_log, dtype=np.int32)
    d['positions'] = np.array([np.asarray(p, dtype=np.float64).reshape(-1)
                               for t in trace for p in t], dtype=np.float64)
    d['Q'] = q
    for k in ('next', 'reward', 'terminal', 'starts', 'coordinates'):
        d['world/' + k] = tabs[k]
    if c['mask']:
        d['action_mask'] = rc.bump_mask(tabs['next'])
    return d


def main() -> None:
    out = {}
    for name in rc.CASES:
        for k, v in run_case(name).items():
            out['%s/%s' % (name, k)] = v
    path = G._out('rollout_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
