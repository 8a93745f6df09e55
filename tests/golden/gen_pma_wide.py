"""Golden traces of PMAMemory and the PMA agent on worlds past 128 states, recorded from the real
reference in float64 (the fixture of the wide form of csrc/pma.hip).

Memory (memory/pma.py): the script of tests/pma_common.py (script_for: about 40 ``store()`` calls
with a repeated (s, a) and a terminal transition, then ``replay()`` calls of length 1, 2, 7 and 32
that cover each switch in turn) on a 12 x 11 world (132 states) and a 17 x 16 world (272 states)
whose start and terminal state lie in the last row, so that the walk and the replays use states
past 127 and past 255 (asserted).  Recorded as gen_pma.py records, but of the SR only the row each
replay reads (its ``current_state``): fifteen 272 x 272 matrices would not fit a fixture.

Agent (agent/pma.py): ``PMA.train`` on the 132-state world with ``mask_actions``, ``gamma_q`` 0.99,
batch 8, 8 trials, no trial timing out (asserted); of the SR after each ``update_sr()`` the rows of
the start and of the terminal state, the two a replay reads.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_pma_wide.py

Reuses the shim and the tape generators of gen_golden.py.  Writes pma_wide_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import SEED, STREAM_ENV, STREAM_POLICY, TapeRNG  # noqa: E402

sys.path.insert(0, os.path.join(G.ROOT, 'tests'))
sys.path.insert(0, os.path.join(G.ROOT, 'cobel-rl_amd'))
import pma_common as pc  # noqa: E402
import pma_wide_common as pw  # noqa: E402


def reference_world(name):
    """The reference's WorldDict of a world of pma_wide_common, checked against the project's tables."""
    from cobel.misc import gridworld_tools as gt
    mine = pw.WORLDS[name]()
    world = gt.make_gridworld(int(mine['height']), int(mine['width']),
                              terminals=list(np.flatnonzero(mine['terminals'])),
                              rewards=np.array([[s, mine['rewards'][s]]
                                                for s in np.flatnonzero(mine['rewards'])]),
                              goals=list(mine['goals']),
                              invalid_transitions=list(mine['invalid_transitions']))
    world['starting_states'] = np.array(mine['starting_states'])
    tabs, sas = pc.tables_of(mine)
    assert np.array_equal(sas, world['sas'])
    assert np.array_equal(tabs['reward'], world['rewards'])
    assert np.array_equal(tabs['terminal'], world['terminals'])
    return world, tabs


def memory_case(wname, inst, n_stores, repeat, start) -> dict:
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    world, tabs = reference_world(wname)
    S = int(world['sas'].shape[0])
    past = 255 if S > 256 else 127
    rm, rp = pc.memory_rngs(SEED, inst)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1, rng=rp), gamma_q=0.99, rng=rm)
    stores = pc.walk_stores(tabs, n_stores, seed=inst, repeat=repeat)
    assert any(r[4] == 0 for r in stores), 'the walk must hold a terminal transition'
    assert any(r[0] > past for r in stores) and any(r[3] > past for r in stores), \
        'the walk must visit states past %d' % past
    ops = pc.script_for(stores, start)
    d = pc.ScriptMemory(mem, pc.masked_actions(tabs),
                        index=lambda m: (m.rng.index, m.policy.rng.index)).run(ops)
    rep = d['replayed']
    assert (rep[:, 1] > past).any() and (rep[:, 4] > past).any(), \
        'the replays must pick states past %d' % past
    states = pw.replay_states(ops)
    assert len(states) == len(d['SR'])
    d['SR'] = np.array([np.zeros(S) if s is None else sr[s] for s, sr in zip(states, d['SR'])])
    d['ops'] = pc.dumps(ops)
    d['cfg'] = np.array([inst], dtype=np.int64)
    return d


def agent_case() -> dict:
    from cobel.agent import PMA
    from cobel.interface import Gridworld
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    world, tabs = reference_world(pw.AGENT_WORLD)
    inst = pw.AGENT_INSTANCE
    start, goal = int(tabs['starts'][0]), int(np.flatnonzero(tabs['terminal'])[0])
    env = Gridworld(world, rng=TapeRNG(SEED, inst, STREAM_ENV))
    rm, rp = pc.memory_rngs(SEED, inst)
    mem = PMAMemory(env.world['sas'], EpsilonGreedy(0.1, rng=rp), gamma_q=0.99, rng=rm)
    tr = pc.new_trace()
    tr['q_replay'] = []

    def on_replay_end(logs):
        first = len(tr['replay_start']) == len(tr['replay_end'])
        tr['replay_start' if first else 'replay_end'].append(pc.rows_of(logs['replay']))
        tr['q_replay'].append(np.array(logs['agent'].Q))
        if not first:
            tr['sr'].append(np.array(logs['agent'].M.SR)[[start, goal]])

    def on_trial_end(logs):
        tr['steps'].append(logs['steps'])
        tr['q_end'].append(np.array(logs['agent'].Q))

    agent = PMA(env.observation_space, env.action_space,
                EpsilonGreedy(0.1, rng=TapeRNG(SEED, inst, STREAM_POLICY)), mem,
                custom_callbacks={'on_replay_end': [on_replay_end], 'on_trial_end': [on_trial_end]})
    agent.mask_actions = True
    agent.train(env, pw.AGENT_TRIALS, pw.AGENT_STEPS, pw.AGENT_BATCH, False)
    steps = np.array(tr['steps'], dtype=np.int64)
    assert (steps < pw.AGENT_STEPS - 1).all(), 'a trial timed out: pick another seed / more steps'
    return {'steps': steps, 'q_end': np.array(tr['q_end']), 'T': np.array(mem.T),
            'rewards': np.array(mem.rewards), 'states': np.array(mem.states).astype(np.int16),
            'terminals': np.array(mem.terminals).astype(np.int8),
            'index': np.array([env.rng.index, agent.policy.rng.index, mem.rng.index,
                               mem.policy.rng.index], dtype=np.int64),
            'sr_rows': np.array(tr['sr']), 'sr_states': np.array([start, goal], dtype=np.int64),
            'q_replay': np.array(tr['q_replay']),
            'replay_start': np.array(tr['replay_start']),
            'replay_end': np.array(tr['replay_end'])}


def main() -> None:
    out = {}
    for name, case in pw.MEMORY_CASES.items():
        for k, v in memory_case(*case).items():
            out['%s/%s' % (name, k)] = v
    for k, v in agent_case().items():
        out['agent_wide/%s' % k] = v
    path = G._out('pma_wide_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
