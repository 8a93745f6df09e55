"""Cases shared by the tests of PMAMemory's observables (compute_gain_batch, compute_gain,
action_probs_batch, update_q: csrc/pma_gain.hip), by tests/golden/gen_pma_gain.py, which records
the real reference on them, and by nothing else.  The NumPy restatement is ``RefPMAMemory`` of
tests/pma_common.py; ``observables`` evaluates a case on any triple of memories with the
reference's methods (the reference's own, or the restatement's), ``device_observables`` on a
device memory of three instances — the same keys, so one comparison serves all.

A case: a world, three memories filled by three different ``walk_stores`` walks (seeds 1, 2, 3:
rewards, successors and terminals differ per instance, a terminal transition among them), an
action mask that leaves every state an action, the Q tables of ``QNAMES`` and the sequences of
``GAIN_SEQS`` / ``UPDATE_SEQS``.  ``gamma`` 0.9 and ``gamma_q`` 0.99 differ, so the two power tables
cannot be swapped unnoticed."""
import functools

import numpy as np

import pma_common as pc
import pma_wide_common as pw
from oracle.ref_loop import RefEpsilonGreedy

N, BASE = 3, 3
MEM_CTR, POL_CTR = 5, 7
GAMMA, GAMMA_Q, EPS = 0.9, 0.99, 0.1
MAX_SEQ = 256                      # cobel_hip.h: COBEL_PMA_MAX_SEQ
STORES = 40
MODES = ('original', 'other')
MASKS = ('plain', 'masked')
QNAMES = ('zero', 'random', 'ties', 'flip', 'stay')
SEQ_Q = ('random', 'flip')         # the tables compute_gain is recorded on
GAIN_SEQS = ('len1', 'len2', 'len7', 'len32', 'repeat', 'terminal', 'lenmax')
UPDATE_SEQS = ('len1', 'len2', 'len7', 'len32', 'repeat', 'terminal', 'lenmax', 'break', 'twice',
               'dead1')
PROB_ROWS, PROB_ACTIONS = (1, 63, 64, 65, 257), (1, 4, 8)


def eight_tabs():
    """9 states x 8 actions by hand: action a < 7 leads a + 1 states on, action 7 stays; state 8
    is terminal and rewarded.  S x A = 72, and ``sum_row`` takes its eight-accumulator path."""
    S, A = 9, 8
    nxt = (np.arange(S)[:, None] + np.arange(A)[None, :] + 1) % S
    nxt[:, 7] = np.arange(S)
    reward, terminal = np.zeros(S), np.zeros(S, dtype=np.int64)
    reward[8], terminal[8] = 10.0, 1
    return {'next': nxt, 'reward': reward, 'terminal': terminal, 'starts': np.array([0])}


def one_tabs():
    """A chain of six states with ONE action; the last state is terminal and rewarded."""
    S = 6
    nxt = np.minimum(np.arange(S) + 1, S - 1)[:, None]
    reward, terminal = np.zeros(S), np.zeros(S, dtype=np.int64)
    reward[5], terminal[5] = 1.0, 1
    return {'next': nxt, 'reward': reward, 'terminal': terminal, 'starts': np.array([0])}


# name: (tables, wide form)
WORLDS = {
    'small_3x4': (lambda: pc.tables_of(pc.small_world())[0], False),     # S x A = 48
    'demo_5x5': (lambda: pc.tables_of(pc.demo_world())[0], False),       # 100
    'eight_9x8': (eight_tabs, False),                                    # 72, A == 8
    'one_6x1': (one_tabs, False),                                        # A == 1
    'wide_132': (lambda: pc.tables_of(pw.world_132())[0], True),         # past the narrow form
}


def exp(row) -> dict:
    s, a, r, ns, t = row
    return {'state': int(s), 'action': int(a), 'reward': float(r), 'next_state': int(ns),
            'terminal': int(t)}


def q_tables(S: int, A: int, seed: int) -> dict:
    r = np.random.default_rng(seed)
    out = {'zero': np.zeros((S, A)),                        # every row an exact tie
           'random': r.normal(size=(N, S, A))}              # one table per instance
    ties = r.normal(size=(S, A))
    top = np.abs(ties).max() + 1.0
    ties[0, 0] = ties[0, A - 1] = top                       # two actions tie at the top
    ties[1, :] = 0.5                                        # all actions tie
    ties[2, 0] = ties[2, A // 2] = -top                     # a tie that is not at the top
    ties[S - 1, :] = -0.25
    out['ties'] = ties
    # action 0 is greedy by a little: a rewarded backup of another action makes that one greedy
    flip = np.full((S, A), 0.1)
    flip[:, 0] = 0.2
    out['flip'] = flip
    # action 0 is greedy by far: no one-step backup changes the policy, every gain is clipped
    stay = np.full((S, A), 0.1)
    stay[:, 0] = 100.0
    out['stay'] = stay
    return out


def sequences(tabs) -> dict:
    """Hand-built n-step updates from a long walk: its non-terminal experiences in walk order and
    its first terminal one (``terminal`` = 0)."""
    rows = pc.walk_stores(tabs, 900, seed=7)
    live = [r for r in rows if r[4] == 1]
    dead = [r for r in rows if r[4] == 0][0]
    assert len(live) >= MAX_SEQ
    seqs = {'len%d' % n: live[:n] for n in (1, 2, 7, 32)}
    seqs['lenmax'] = live[:MAX_SEQ]
    seqs['repeat'] = [live[0], live[1], live[0]]            # a state (and its action) comes back
    # ends in a terminal step: bootstrap 0 (and update_q, which looks ahead from step 0, breaks)
    seqs['terminal'] = [live[0], live[1], dead]
    seqs['break'] = [live[0], dead, live[1]]                # update_q: an intermediate terminal
    seqs['twice'] = [live[0], live[0]]                      # update_q writes one (s, a) twice
    seqs['dead1'] = [dead]                                  # one terminal step: applied, bootstrap 0
    return {k: [exp(r) for r in v] for k, v in seqs.items()}


@functools.lru_cache(maxsize=None)
def build(name: str) -> dict:
    make, wide = WORLDS[name]
    tabs = make()
    nxt = np.asarray(tabs['next']).astype(np.int64)
    S, A = nxt.shape
    stores = [pc.walk_stores(tabs, STORES, seed=i + 1) for i in range(N)]
    assert all(any(r[4] == 0 for r in rows) for rows in stores), 'a walk without a terminal step'
    return {'name': name, 'tabs': tabs, 'next': nxt, 'S': S, 'A': A, 'wide': wide,
            'sas': pc.sas_of(nxt), 'stores': stores, 'mask': pc.masked_actions(tabs),
            'Q': q_tables(S, A, 100 + len(name)), 'seqs': sequences(tabs)}


def q_of(case: dict, qname: str, i: int):
    Q = case['Q'][qname]
    return Q[i] if Q.ndim == 3 else Q


def seq_names(qname: str):
    """(the longest sequence is scored on one table only: the restatement takes its time)"""
    return GAIN_SEQS if qname == 'random' else GAIN_SEQS[:-1]


def restatement_memories(case: dict, mode: str = 'original') -> list:
    mems = []
    for i in range(N):
        m = pc.RefPMAMemory(case['sas'], RefEpsilonGreedy(EPS, None), gamma=GAMMA, gamma_q=GAMMA_Q)
        m.min_gain_mode = mode
        for row in case['stores'][i]:
            m.store(exp(row))
        mems.append(m)
    return mems


def observables(case: dict, memories, real: bool = False) -> dict:
    """``memories(mode)`` -> the three filled memories.  ``real``: they are the reference's (whose
    compute_gain takes a list of updates and whose probabilities are ``action_probs_batch``)."""
    A = case['A']
    out = {}
    by_mode = {mode: memories(mode) for mode in MODES}
    mems = by_mode['original']
    for mname in MASKS:
        mask = case['mask'] if mname == 'masked' else None
        for qname in QNAMES:
            out['gain_batch/%s/%s' % (mname, qname)] = np.array(
                [m.compute_gain_batch(np.array(q_of(case, qname, i)), mask)
                 for i, m in enumerate(mems)])
        for mode in MODES:
            for qname in SEQ_Q:
                ups = [case['seqs'][k] for k in seq_names(qname)]
                rows = []
                for i, m in enumerate(by_mode[mode]):
                    Q = np.array(q_of(case, qname, i))
                    rows.append(m.compute_gain(Q, mask, ups) if real
                                else [m.compute_gain(Q, mask, u) for u in ups])
                out['gain_seq/%s/%s/%s' % (mode, mname, qname)] = np.array(rows, dtype=np.float64)
        Q0 = np.tile(q_of(case, 'ties', 0), (A, 1))
        tiled = np.tile(mask, (A, 1)) if mask is not None else None
        out['probs/' + mname] = np.array(mems[0].action_probs_batch(Q0, tiled) if real
                                         else mems[0]._probs_batch(Q0, tiled))
    for sname in UPDATE_SEQS:
        out['update_q/' + sname] = np.array(
            [m.update_q(np.array(q_of(case, 'random', i)), case['seqs'][sname])
             for i, m in enumerate(mems)])
    return out


@functools.lru_cache(maxsize=None)
def expected(name: str) -> dict:
    """The restatement's word on a case, computed once per process."""
    case = build(name)
    return observables(case, lambda mode: restatement_memories(case, mode))


def prob_case(rows: int, A: int, masked: bool):
    """A [rows, A] table with planted ties and, if asked, a mask that leaves every row an action."""
    r = np.random.default_rng(1000 * rows + 10 * A + int(masked))
    q = np.round(r.normal(size=(rows, A)), 1)               # one decimal: exact ties abound
    q[0, :] = 0.0
    mask = None
    if masked:
        mask = r.random((rows, A)) < 0.6
        mask[np.arange(rows), r.integers(0, A, rows)] = True
    return q, mask


def probs_restated(q, mask, eps: float = EPS):
    return pc.RefPMAMemory._probs_batch(_PolicyOnly(eps), q, mask)


class _PolicyOnly:
    """What ``RefPMAMemory._probs_batch`` reads of a memory."""

    def __init__(self, eps):
        self.policy = RefEpsilonGreedy(eps, None)


# -- the device side ---------------------------------------------------------------------------------
def device_memory(case: dict, seed: int, mode: str = 'original', n: int = N, frames=None):
    """A bound device memory of ``n`` instances holding the case's stores (instance i: walk
    i % 3).  ``frames``: called with the memory right after ``bind`` (tests that frame its tables)."""
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(case['sas'], EpsilonGreedy(EPS), gamma=GAMMA, gamma_q=GAMMA_Q, wide=case['wide'])
    mem.min_gain_mode = mode
    mem.bind(n, seed=seed, instance_base=BASE)
    if frames is not None:
        frames(mem)
    walks = [case['stores'][i % N] for i in range(n)]
    for k in range(STORES):
        pick = [w[k] for w in walks]
        mem.store({'state': [r[0] for r in pick], 'action': [r[1] for r in pick],
                   'reward': [r[2] for r in pick], 'next_state': [r[3] for r in pick],
                   'terminal': [r[4] for r in pick]})
    # counters somewhere in the middle of their streams: none of the new calls may move them
    mem.counter.fill_(MEM_CTR)
    mem._policy_counter().fill_(POL_CTR)
    return mem


def assert_counters_rest(mem):
    assert bool((mem.counter == MEM_CTR).all()), 'the memory drew a number'
    assert bool((mem.policy.counter == POL_CTR).all()), "the memory's policy drew a number"


def host(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def device_observables(case: dict, seed: int, as_tensor: bool = False) -> dict:
    """The keys of ``observables`` from the device memory's four methods.  ``as_tensor``: the Q
    tables go in as device tensors, not as NumPy arrays."""
    import torch
    A = case['A']
    out = {}
    by_mode = {mode: device_memory(case, seed, mode) for mode in MODES}
    mem = by_mode['original']
    give = (lambda a: torch.as_tensor(a, device=mem.device)) if as_tensor else (lambda a: a)
    for mname in MASKS:
        mask = case['mask'] if mname == 'masked' else None
        for qname in QNAMES:
            out['gain_batch/%s/%s' % (mname, qname)] = host(
                mem.compute_gain_batch(give(case['Q'][qname]), mask))
        for mode in MODES:
            for qname in SEQ_Q:
                ups = [case['seqs'][k] for k in seq_names(qname)]
                out['gain_seq/%s/%s/%s' % (mode, mname, qname)] = host(
                    by_mode[mode].compute_gain(give(case['Q'][qname]), mask, ups))
        Q0 = np.tile(q_of(case, 'ties', 0), (A, 1))
        tiled = np.tile(mask, (A, 1)) if mask is not None else None
        out['probs/' + mname] = host(mem.action_probs_batch(give(Q0), tiled))
    for sname in UPDATE_SEQS:
        Q = np.array(case['Q']['random'])
        if as_tensor:
            Q = torch.as_tensor(Q, device=mem.device)
        back = mem.update_q(Q, case['seqs'][sname])
        assert back is Q, 'update_q returns the table it was given, updated in place'
        out['update_q/' + sname] = host(back)
    for m in by_mode.values():
        assert_counters_rest(m)
    return out


def per_instance(seqs) -> list:
    """One sequence per instance (lists of experience dicts, of different lengths) as ONE update
    whose values are [N] arrays; a state of -1 ends an instance's sequence."""
    none = {'state': -1, 'action': 0, 'reward': 0.0, 'next_state': 0, 'terminal': 1}
    longest = max(len(u) for u in seqs)
    return [{k: [(u[j] if j < len(u) else none)[k] for u in seqs] for k in pc.KEYS}
            for j in range(longest)]


def assert_same(got: dict, want: dict, what: str = ''):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError('%s %s differs first at %s: %r != %r (%d of %d entries differ)'
                                 % (what, k, bad.tolist(), g[tuple(bad)], w[tuple(bad)],
                                    int((g != w).sum()), g.size))
