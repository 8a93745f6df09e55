"""Golden traces of PMAMemory and the PMA agent, recorded from the real reference in float64.

Memory on its own (memory/pma.py): scripts of calls (tests/pma_common.py: script_for) on the demo's
5 x 5 world and on a 3 x 4 world with one wall (S x A = 48, less than one wavefront) — a seeded
walk of about 40 ``store()`` calls with a repeated (s, a) and a terminal transition, then
``replay()`` calls of length 1, 2, 7 and 32 that cover each switch in turn.  Recorded: the calls, T,
the SR in force at each replay, every returned update, the returned Q, the generator indices of
both streams after each call and, for ``current_state=None``, the need vector.

Agent (agent/pma.py): ``PMA.train`` on the demo world with ``mask_actions``, ``gamma_q`` 0.99, batch
8, 12 trials, no trial timing out (asserted); per trial the SR after ``update_sr()``, Q after each
replay, ``logs['replay']`` at both replays and the latency.  One short case with ``no_replay``.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_pma.py

Reuses the shim and the tape generators of gen_golden.py.  Writes pma_traces.npz.
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

# name: (world, instance, stores, repeat, start state)
MEMORY_CASES = {
    'mem_demo_5x5': ('demo_5x5', 3, 40, (6, 3), 12),
    'mem_small_3x4': ('small_3x4', 1, 40, (9, 2), 8),
}
AGENT_INSTANCE, AGENT_TRIALS, AGENT_STEPS, AGENT_BATCH = 0, 12, 400, 8


def reference_world(name):
    """The reference's WorldDict of a world of pma_common, checked against the project's tables."""
    from cobel.misc import gridworld_tools as gt
    mine = pc.WORLDS[name]()
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
    rm, rp = pc.memory_rngs(SEED, inst)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1, rng=rp), gamma_q=0.99, rng=rm)
    stores = pc.walk_stores(tabs, n_stores, seed=inst, repeat=repeat)
    assert any(r[4] == 0 for r in stores), 'the walk must hold a terminal transition'
    ops = pc.script_for(stores, start)
    d = pc.ScriptMemory(mem, pc.masked_actions(tabs),
                        index=lambda m: (m.rng.index, m.policy.rng.index)).run(ops)
    d['ops'] = pc.dumps(ops)
    d['cfg'] = np.array([inst], dtype=np.int64)
    return d


def agent_case(no_replay: bool, trials: int) -> dict:
    from cobel.agent import PMA
    from cobel.interface import Gridworld
    from cobel.memory import PMAMemory
    from cobel.policy import EpsilonGreedy
    world, _ = reference_world('demo_5x5')
    inst = AGENT_INSTANCE
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
            tr['sr'].append(np.array(logs['agent'].M.SR))

    def on_trial_end(logs):
        tr['steps'].append(logs['steps'])
        tr['q_end'].append(np.array(logs['agent'].Q))

    agent = PMA(env.observation_space, env.action_space,
                EpsilonGreedy(0.1, rng=TapeRNG(SEED, inst, STREAM_POLICY)), mem,
                custom_callbacks={'on_replay_end': [on_replay_end], 'on_trial_end': [on_trial_end]})
    agent.mask_actions = True
    agent.train(env, trials, AGENT_STEPS, AGENT_BATCH, no_replay)
    steps = np.array(tr['steps'], dtype=np.int64)
    assert (steps < AGENT_STEPS - 1).all(), 'a trial timed out: pick another seed / more steps'
    out = {'steps': steps, 'q_end': np.array(tr['q_end']), 'T': np.array(mem.T),
           'rewards': np.array(mem.rewards), 'states': np.array(mem.states).astype(np.int16),
           'terminals': np.array(mem.terminals).astype(np.int8),
           'index': np.array([env.rng.index, agent.policy.rng.index, mem.rng.index,
                              mem.policy.rng.index], dtype=np.int64)}
    if not no_replay:
        out.update({'sr': np.array(tr['sr']), 'q_replay': np.array(tr['q_replay']),
                    'replay_start': np.array(tr['replay_start']),
                    'replay_end': np.array(tr['replay_end'])})
    return out


def main() -> None:
    out = {}
    for name, case in MEMORY_CASES.items():
        for k, v in memory_case(*case).items():
            out['%s/%s' % (name, k)] = v
    for name, args in (('agent_demo', (False, AGENT_TRIALS)), ('agent_no_replay', (True, 4))):
        for k, v in agent_case(*args).items():
            out['%s/%s' % (name, k)] = v
    path = G._out('pma_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
