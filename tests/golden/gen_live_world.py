"""Golden traces of worlds EDITED between calls, recorded from the real reference.

The reference reads ``world['sas'] / ['rewards'] / ['terminals'] / ['starting_states']`` on every
``step()`` and ``reset()`` (interface/gridworld.py:115-126, :142), so a user trains, moves the
reward or the start box or closes a passage, and trains again.  Every case here is a run in
phases with an edit of the world in front of every phase but the first; the edits are stored as
data (the tables as they stand after the edit) so that the tests replay them.

    COBEL_REFERENCE_SRC=<reference>/src python tests/golden/gen_live_world.py

Reuses the shim, the tape generators and the tracer of gen_golden.py; float32 tables as in
gen_dynaq / gen_sr.  Writes live_world_traces.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (loads the reference)
from gen_golden import (SEED, STREAM_ENV, STREAM_MEMORY, STREAM_POLICY, SR, DynaQ,  # noqa: E402
                        EpsilonGreedy, Gridworld, TapeRNG, Tracer, gt)


def edit(rewards=None, terminals=None, starts=None, moves=None, slip=0.0) -> dict:
    """``rewards`` / ``terminals``: {state: value}; ``starts``: the new list; ``moves``:
    {(state, action): successor} — one-hot rows of sas rewritten; ``slip``: every row becomes a
    distribution (gen_golden.slippery) and ``deterministic`` goes off."""
    return dict(rewards=rewards or {}, terminals=terminals or {}, starts=starts, moves=moves or {},
                slip=slip)


def apply_edit(world, e) -> None:
    for s, v in e['rewards'].items():
        world['rewards'][s] = v
    for s, v in e['terminals'].items():
        world['terminals'][s] = v
    if e['starts'] is not None:
        world['starting_states'] = np.array(e['starts'])
    for (s, a), ns in e['moves'].items():
        world['sas'][s, a] = 0.0
        world['sas'][s, a, ns] = 1.0
    if e['slip']:
        G.slippery(world, e['slip'])


def tables(world) -> dict:
    """The world as it stands, in the form the tests replay it from."""
    return dict(next=np.argmax(world['sas'], axis=2).astype(np.uint16),
                rewards=np.array(world['rewards'], dtype=np.float64),        # (copies: edits are in place)
                terminals=np.asarray(world['terminals']).astype(np.uint8),
                starts=np.asarray(world['starting_states']).astype(np.uint16))


# The reversal of the issue: reward and terminal move to the opposite corner, a penalty turns up,
# the start box moves.
REVERSAL = edit(rewards={7: 0.0, 56: 1.0, 30: -0.25}, terminals={7: 0, 0: 1}, starts=[63, 5, 40])
# Detour: the column x = 5 between the start box and the goal closes except at the bottom row
# (moves right from x = 4 and left from x = 6 stay put in rows 0 .. 6).
DETOUR = edit(moves={**{(8 * y + 4, 2): 8 * y + 4 for y in range(7)},
                     **{(8 * y + 6, 0): 8 * y + 6 for y in range(7)}})

CASES = {
    # name: (agent, instance, B, [(trials, steps, edit in front of the phase)])
    'dynaq_reversal': ('dynaq', 3, 8, [(12, 60, None), (12, 60, REVERSAL)]),
    'dynaq_detour': ('dynaq', 5, 8, [(10, 60, None), (10, 60, REVERSAL), (10, 60, DETOUR)]),
    # rewarded states 1 -> 3 -> 9: the three forms of the sparse-reward SR kernel
    'sr_rewards_1_3_9': ('sr', 1, 0, [
        (10, 60, edit(rewards={56: 0.0, 30: 0.0})),
        (10, 60, edit(rewards={56: -0.5, 30: 0.25}, starts=[63, 5, 40])),
        (10, 60, edit(rewards={1: 0.125, 9: -0.125, 18: 0.5, 40: 0.0625, 47: -1.0, 61: 2.0}))]),
    'dynaq_turns_slippery': ('dynaq', 2, 8, [(10, 60, None), (10, 60, edit(slip=0.2))]),
    'sr_turns_slippery': ('sr', 4, 0, [(8, 60, None), (8, 60, edit(slip=0.3, starts=[63, 32]))]),
}


def run_case(kind, inst, B, phases) -> dict:
    world = G.walls_8x8()
    first = phases[0][2]
    if first is not None:                 # (an edit in front of phase 0 shapes the initial world)
        apply_edit(world, first)
    env = Gridworld(world, rng=TapeRNG(SEED, inst, STREAM_ENV, double_sub=1))
    pol = EpsilonGreedy(0.1, rng=TapeRNG(SEED, inst, STREAM_POLICY))
    if kind == 'sr':
        ag = SR(env.observation_space, env.action_space, pol)
        ag.SR = ag.SR.astype(np.float32)
        ag.rewards = ag.rewards.astype(np.float32)
    else:
        ag = DynaQ(env.observation_space, env.action_space, pol)
        ag.M.rng = TapeRNG(SEED, inst, STREAM_MEMORY)
        ag.Q = ag.Q.astype(np.float32)
        ag.M.rewards = ag.M.rewards.astype(np.float32)
    tr = Tracer(None)
    ag.callbacks.custom_callbacks = {k: list(v) for k, v in tr.callbacks().items()}
    for k in ('on_trial_begin', 'on_step_begin'):
        ag.callbacks.custom_callbacks.setdefault(k, [])
    d, ends = {}, []
    for p, (trials, steps, e) in enumerate(phases):
        if p and e is not None:
            apply_edit(world, e)
        for k, v in tables(world).items():
            d['phase%d/%s' % (p, k)] = v
        d['phase%d/slip' % p] = np.float64(e['slip'] if e else 0.0)
        if kind == 'sr':
            ag.train(env, trials, steps)
            d['phase%d/SR' % p] = np.array(ag.SR, dtype=np.float64)
            d['phase%d/RW' % p] = np.array(ag.rewards, dtype=np.float64)
            d['phase%d/T' % p] = np.argmax(ag.transitions, axis=-1).astype(np.int16)
        else:
            ag.train(env, trials, steps, B)
            d['phase%d/Q' % p] = np.array(ag.Q, dtype=np.float64)
            d['phase%d/M_rewards' % p] = np.array(ag.M.rewards, dtype=np.float64)
            d['phase%d/M_states' % p] = ag.M.states.astype(np.int16)
            d['phase%d/M_terminals' % p] = ag.M.terminals.astype(np.int8)
        ends.append(len(tr.sarsn))
    t = tr.pack()
    t.pop('td', None)
    t.pop('Q_trial', None)
    d.update(t)
    d['step_ends'] = np.array(ends, dtype=np.int64)          # env steps at the end of each phase
    d['cfg'] = np.array([inst, B, len(phases)], dtype=np.int64)
    d['phases'] = np.array([(tr_, st) for tr_, st, _ in phases], dtype=np.int64)
    d['agent'] = np.array(kind)
    return d


def hex_tables(nodes, starts) -> dict:
    """A node dictionary and a start list as index tables (rows in the order of the dictionary)."""
    ids = list(nodes.keys())
    index = {k: i for i, k in enumerate(ids)}
    return dict(next=np.array([[index[m] for m in nodes[k]['neighbors']] for k in ids], dtype=np.uint16),
                rewards=np.array([nodes[k]['reward'] for k in ids], dtype=np.float64),
                terminals=np.array([bool(nodes[k]['terminal']) for k in ids]).astype(np.uint8),
                starts=np.array([index[k] for k in starts], dtype=np.uint16))


def run_hex_case(inst=4, B=8, phases=((15, 40), (15, 40), (15, 40))) -> dict:
    """QAgent on the hexagonal Topology of gen_qagent_topology (six actions, goal at node '7'):
    nodes' reward / terminal edited in place and starting_nodes replaced between the phases, which
    Topology.step / reset read anew on every call (interface/topology.py:126-172)."""
    from cobel.agent.q import QAgent
    from cobel.interface import Topology
    from cobel.misc import topology_tools as tt
    nodes, starts = tt.hexagonal(5, (0.0, 2.0), 3.0, '7')
    ids = list(nodes.keys())
    env = Topology(nodes, starts, None, rng=TapeRNG(SEED, inst, STREAM_ENV))
    pol = EpsilonGreedy(0.1, rng=TapeRNG(SEED, inst, STREAM_POLICY))
    ag = QAgent(env.observation_space, env.action_space, pol, rng=TapeRNG(SEED, inst, STREAM_MEMORY))
    key = {tuple(np.array(nodes[k]['pose']).flatten()): i for i, k in enumerate(ids)}
    for k in key:
        ag.Q[k] = np.zeros(6, dtype=np.float32)
    sarsn, steps_log = [], []
    ag.callbacks.custom_callbacks = {
        'on_step_end': [lambda logs: sarsn.append((key[logs['state']], logs['action'], logs['reward'],
                                                   key[logs['next_state']], logs['terminal']))],
        'on_trial_end': [lambda logs: steps_log.append(logs['steps'])],
        'on_trial_begin': [], 'on_step_begin': []}
    far, mid = ids[-2], ids[len(ids) // 2]
    d, ends = {}, []
    for p, (trials, steps) in enumerate(phases):
        if p == 1:        # the goal moves to the far side, a penalty turns up, another start box
            nodes['7'].update(reward=0.0, terminal=False)
            nodes[far].update(reward=2.0, terminal=True)
            nodes[mid]['reward'] = -0.5
            env.starting_nodes = ['7', ids[1], ids[len(ids) // 3 + 2]]
        if p == 2:        # two goals, the penalty becomes a trap, one start node
            nodes['7'].update(reward=1.0, terminal=True)
            nodes[mid]['terminal'] = True
            env.starting_nodes = [ids[len(ids) // 3 + 2]]
        for k, v in hex_tables(nodes, env.starting_nodes).items():
            d['phase%d/%s' % (p, k)] = v
        ag.train(env, trials, steps, B)
        Q = np.zeros((len(ids), 6))
        for k, row in ag.Q.items():
            Q[key[k]] = row
        d['phase%d/Q' % p] = Q
        d['phase%d/log_len' % p] = np.int64(len(ag.M))
        ends.append(len(sarsn))
    a = np.array(sarsn, dtype=np.float64).reshape(-1, 5)
    d.update(state=a[:, 0].astype(np.int16), action=a[:, 1].astype(np.int8), reward=a[:, 2],
             next_state=a[:, 3].astype(np.int16), nonterminal=a[:, 4].astype(np.int8),
             steps=np.array(steps_log, dtype=np.int32), step_ends=np.array(ends, dtype=np.int64),
             cfg=np.array([inst, B, len(phases)], dtype=np.int64),
             phases=np.array(phases, dtype=np.int64), agent=np.array('q_hex'),
             ids=np.array(ids))
    return d


def env_kat() -> dict:
    """``step`` / ``reset`` alone, with edits between single steps: rows (op, arg, state, reward,
    end); op 0 = reset, 1 = step(arg), 2 = edit number arg applied (its row repeats the state)."""
    world = G.walls_8x8()
    env = Gridworld(world, rng=TapeRNG(SEED, 6, STREAM_ENV, double_sub=1))
    edits = [REVERSAL, DETOUR, edit(rewards={62: 3.0}, terminals={62: 1}, starts=[61]),
             edit(terminals={62: 0}, rewards={62: 0.0}, starts=[55, 61, 47])]
    rng = np.random.default_rng(11)
    rows, d, k = [], {}, 0
    for i in range(160):
        if i and i % 32 == 0:
            apply_edit(world, edits[k])
            for key, v in tables(world).items():
                d['edit%d/%s' % (k, key)] = v
            rows.append((2, k, env.current_state, 0.0, 0))
            k += 1
        if i % 32 in (1, 17) or (rows and rows[-1][4]):
            s, _ = env.reset()
            rows.append((0, 0, s, 0.0, 0))
        # (right after an edit of the start list: mostly moves towards the edited cells)
        a = int(rng.integers(4))
        s, r, end, _, _ = env.step(a)
        rows.append((1, a, s, float(r), int(end)))
    d['rows'] = np.array(rows, dtype=np.float64)
    d['instance'] = np.int64(6)
    return d


def main() -> None:
    out = {}
    for name, (kind, inst, B, phases) in CASES.items():
        for k, v in run_case(kind, inst, B, phases).items():
            out['%s/%s' % (name, k)] = v
    for k, v in run_hex_case().items():
        out['qagent_hex/%s' % k] = v
    for k, v in env_kat().items():
        out['env_kat/%s' % k] = v
    path = G._out('live_world_traces.npz')
    np.savez_compressed(path, **out)
    print('%-24s %8d B' % (os.path.basename(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
