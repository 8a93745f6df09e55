"""Shared by the live-world tests: the golden cases of tests/golden/gen_live_world.py (runs in
phases, the world edited in front of every phase; the tables after each edit are stored) and the
ways a test replays an edit on an oracle world and on a product world."""
import os

import numpy as np

from conftest import GOLDEN

DETERMINISTIC = ('dynaq_reversal', 'dynaq_detour', 'sr_rewards_1_3_9')
SLIPPERY = ('dynaq_turns_slippery', 'sr_turns_slippery')


def load():
    return np.load(os.path.join(GOLDEN, 'live_world_traces.npz'))


def case(D, name):
    inst, B, n_phases = [int(x) for x in D[name + '/cfg']]
    phases = [(int(t), int(s)) for t, s in D[name + '/phases']]
    assert len(phases) == n_phases
    return str(D[name + '/agent']), inst, B, phases


def tables(D, name, p, prefix='phase'):
    """Tables after the edit in front of phase p, keyed as the oracles take them (``sas``: dense
    distribution rows where the phase is slippery)."""
    key = '%s/%s%d/' % (name, prefix, p)
    t = dict(next=D[key + 'next'], reward=D[key + 'rewards'], terminal=D[key + 'terminals'],
             starts=D[key + 'starts'])
    slip = float(D[key + 'slip']) if key + 'slip' in D.files else 0.0
    if slip:
        t['sas'] = slippery_sas(t['next'], slip)
    return t


def slippery_sas(det, p_slip):
    """gen_golden.slippery on the table ``det``: the intended move keeps 1 - p_slip, each
    perpendicular move gets p_slip / 2 (same additions in the same order)."""
    S = det.shape[0]
    sas = np.zeros((S, 4, S))
    for s in range(S):
        for a in range(4):
            sas[s, a, det[s, a]] += 1.0 - p_slip
            sas[s, a, det[s, (a + 1) % 4]] += p_slip / 2
            sas[s, a, det[s, (a + 3) % 4]] += p_slip / 2
    return sas


def edit_world(world, t) -> None:
    """Replay an edit on a product world the ways a user makes one: rewards and terminals IN
    PLACE, the start list as a REPLACED entry, moved transitions as rewritten one-hot rows of the
    materialised dense ``sas``, slippery floors as a replaced ``sas`` with ``deterministic`` off."""
    world['rewards'][:] = t['reward']
    world['terminals'][:] = t['terminal']
    world['starting_states'] = np.array(t['starts'], dtype=int)
    if 'sas' in t:
        world['sas'] = t['sas'].copy()
        world['deterministic'] = False
        return
    cur = np.asarray(world['next'])
    rows = np.argwhere(cur != t['next'])
    if len(rows):
        sas = world['sas']          # materialises the dense tensor; it is the source of truth now
        for s, a in rows:
            sas[s, a] = 0.0
            sas[s, a, int(t['next'][s, a])] = 1.0


def product_world(tab, t0):
    """A product World of the golden world ``tab`` carrying the tables of phase 0."""
    from conftest import as_world
    w = as_world(tab)
    w['next'] = np.array(t0['next'], dtype=np.uint16)
    w['rewards'] = np.array(t0['reward'], dtype=float)
    w['terminals'] = np.array(t0['terminal'], dtype=int)
    w['starting_states'] = np.array(t0['starts'], dtype=int)
    return w


def unpack_model(raw):
    """cobel_pack_model words -> (reward estimates, successors, non-terminal flags)."""
    r = (raw & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64)
    return r, ((raw >> 32) & 0xFFFF).astype(np.int64), ((raw >> 48) & 1).astype(np.int64)


HEX = 'qagent_hex'


def hex_nodes():
    """The hexagonal graph of the golden case (six actions, goal at node '7') as the product's own
    builder makes it; the node order must be the one the golden's index tables use."""
    from cobel_amd.misc.topology_tools import hexagonal
    nodes, starts = hexagonal(5, (0.0, 2.0), 3.0, '7')
    return nodes, starts


def edit_nodes(env, ids, t) -> None:
    """Replay an edit on a Topology the way a user makes one: every node's reward and terminal
    flag IN PLACE in the node dictionary, ``starting_nodes`` REPLACED."""
    for i, k in enumerate(ids):
        env.nodes[k]['reward'] = float(t['reward'][i])
        env.nodes[k]['terminal'] = bool(t['terminal'][i])
    env.starting_nodes = [ids[int(j)] for j in t['starts']]
