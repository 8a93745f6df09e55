"""PMA's parameter sets inside sentinel frames (tests/frames_common.py): ``param_sets``,
``param_index`` and the power tables of a launch with sets, framed, in every entry point that reads
them — cobel_pma_trial, cobel_pma_update_sr (the LDS kernel and the blocked kernels),
cobel_pma_replay, cobel_pma_store, cobel_pma_gain_batch, cobel_pma_gain_seq and
cobel_pma_update_q_sets with both pairs.  No guard byte changes, the framed tables are unchanged,
and every result equals the plain run's bit for bit.

The guards hold values that would show in a result: ``BIG`` in the doubles of a set and of a power
table, set 2 in the index (the first instance's set is 0, the last one's 1).  The framed run also
carries an index EQUAL to ``n_param_sets`` for an instance of the last set: the kernels clamp it,
so nothing outside the table of sets is read and the results are still the plain run's."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
import pma_common as pc
import pma_sets_common as sc

pytestmark = pytest.mark.gpu

NAME = 'demo_5x5'
TABLES = ('sets', 'index', 'gamma_pow', 'gamma_q_pow', 'agent_pow')
POISON = {'sets': fc.BIG, 'index': 2, 'gamma_pow': fc.BIG, 'gamma_q_pow': fc.BIG,
          'agent_pow': fc.BIG}
LONGEST = 40                   # the longest replay / sequence below: the tables are built for it


def everything(framed: bool, blocked_sr, monkeypatch) -> dict:
    from cobel_amd import _lib
    cols = sc.columns(sc.SETS3, sc.WHICH7)
    agent_part = (cols['alpha'], cols['agent_gamma'], cols['epsilon'])
    env, agent, mem = sc.build(NAME, sc.N, sc.BASE, cols)
    _, tabs, sas, _ = sc.world_of(NAME)
    agent.train(env, 1, 10, 4)                       # builds the agent's sets
    mem._mem(length=LONGEST, agent=agent_part)       # ... with tables for the longest length
    mem._mem(length=LONGEST)                         # ... and the memory's own
    frames, kept = fc.Frames(), {}
    if framed:
        for who in ('agent', 'memory'):
            held = mem._psets[who]
            assert held['n'] == 3
            for key in TABLES:
                # the sets are a byte tensor: framed as the doubles they hold
                if key == 'sets':
                    held[key] = held[key].view(torch.float64)
                if key == 'index':
                    # the last instance of the last set (np.unique's order) points one past it
                    idx = held[key].cpu().numpy().view(np.uint16).copy()
                    last = int(np.flatnonzero(idx == 2)[-1])
                    idx[last] = 3
                    held[key] = torch.as_tensor(idx.view(np.int16), device=held[key].device)
                kept[who, key] = held[key].clone()
                frames.swap(held, key, POISON[key])
    if blocked_sr:
        monkeypatch.setenv('COBEL_DEBUG', '1')
        monkeypatch.setenv('COBEL_DEBUG_PMA_SR', 'blocked')
    try:
        agent.train(env, 2, 20, 8)                   # cobel_pma_trial, _update_sr, _replay
    finally:
        if blocked_sr:
            monkeypatch.delenv('COBEL_DEBUG_PMA_SR')
            monkeypatch.delenv('COBEL_DEBUG')
    out = sc.state_of(env, agent, mem, 3)
    rows = pc.walk_stores(tabs, 12, seed=3)
    for k in range(len(rows)):                       # cobel_pma_store
        pick = [rows[max(k - i, 0)] for i in range(sc.N)]
        mem.store({'state': [r[0] for r in pick], 'action': [r[1] for r in pick],
                   'reward': [r[2] for r in pick], 'next_state': [r[3] for r in pick],
                   'terminal': [r[4] for r in pick]})
    mem.update_sr()                                  # cobel_pma_update_sr (the LDS kernel)
    ups, q = mem.replay(agent._q, None, LONGEST, 12)   # cobel_pma_replay, the longest
    out['replay'] = np.array([pc.rows_of(u) for u in ups])
    out['q_replay'] = q.cpu().numpy()
    out['gain_batch'] = mem.compute_gain_batch(q, None).cpu().numpy()
    keys = ('state', 'action', 'reward', 'next_state', 'terminal')
    seq = [dict(zip(keys, (int(r[0]), int(r[1]), float(r[2]), int(r[3]), 1)))
           for r in pc.walk_stores(tabs, LONGEST, seed=5)]
    out['gain_seq'] = mem.compute_gain(q, None, [seq[:7], seq]).cpu().numpy()
    out['update_q_memory'] = mem.update_q(q.clone(), seq).cpu().numpy()
    agent.update_q(seq)                              # cobel_pma_update_q_sets, the agent's pair
    torch.cuda.synchronize()
    out['update_q_agent'] = agent._q.cpu().numpy()
    for key in mem._dev:
        out['end_' + key] = mem._dev[key].cpu().numpy()
    if framed:
        frames.check()
        for (who, key), t in kept.items():
            assert fc.same_bits(mem._psets[who][key], t), (who, key)
    assert mem._psets['agent']['gamma_pow'].shape == (3, LONGEST + 1)
    assert mem._mem(length=LONGEST).flags & _lib.PMA_SETS and int(mem._tail.n_param_sets) == 3
    return out


@pytest.mark.parametrize('blocked_sr', [False, True], ids=['lds_sr', 'blocked_sr'])
def test_sets_index_and_power_tables_inside_sentinel_frames(blocked_sr, monkeypatch):
    plain = everything(False, blocked_sr, monkeypatch)
    framed = everything(True, blocked_sr, monkeypatch)
    assert plain['replay'].shape == (sc.N, LONGEST, 5)
    assert not np.array_equal(plain['update_q_agent'][0], plain['update_q_agent'][1])
    fc.assert_same(plain, framed)


def test_an_index_past_the_sets_in_a_hand_built_call():
    """cobel_pma_store with a hand-built struct: two sets inside a frame whose guards hold ``BIG``,
    every index equal to ``n_param_sets``.  The kernel clamps it to the last set: the rewards are
    the last set's, no guard value reaches a table, no guard changes."""
    from cobel_amd import _lib
    from cobel_amd.memory import PMAMemory
    from cobel_amd.memory.pma import RECORD
    from cobel_amd.policy import EpsilonGreedy
    _, tabs, sas, _ = sc.world_of(NAME)
    n = 5
    mem = PMAMemory(sas, EpsilonGreedy(0.1))
    mem.bind(n, seed=sc.SEED, instance_base=sc.BASE)
    sets = (_lib.PMAParamSet * 2)()
    for k, lr in enumerate((0.25, 0.5)):
        _lib.check(_lib.lib().cobel_pma_param_set_fill(
            C.byref((C.c_double * 7)(lr, 0.9, 0.5, 0.9, 0.99, 1e-6, 0.1)), 0.9, 0.99, 0.1,
            C.byref(sets[k])))
    frames = fc.Frames()
    raw = torch.as_tensor(np.frombuffer(sets, dtype=np.float64).copy(), device=mem.device)
    sets_d = frames.add('sets', raw, fc.BIG)
    index_d = frames.add('index', torch.full((n,), 2, dtype=torch.int16, device=mem.device), 2)
    rec = np.zeros(n, dtype=RECORD)
    rec['state'], rec['action'], rec['reward'], rec['next_state'], rec['terminal'] = 12, 1, 8.0, 7, 1
    exps = torch.as_tensor(rec.view(np.uint8), device=mem.device)
    m = mem._mem()                # the head of mem._tail, a cobel_pma_mem_sets_t
    x = mem._tail
    x.param_sets, x.param_index, x.n_param_sets = _lib.ptr(sets_d), _lib.ptr(index_d), 2
    m.flags |= _lib.PMA_SETS
    _lib.check(_lib.lib().cobel_pma_store(C.byref(m), _lib.ptr(exps),
                                          _lib.current_stream(mem.device)))
    torch.cuda.synchronize()
    frames.check()
    assert np.array_equal(np.asarray(mem.rewards)[:, 12, 1], np.full(n, 0.0 + 0.5 * (8.0 - 0.0)))
    T = np.asarray(mem.T)
    assert np.isfinite(T).all() and np.abs(T).max() <= 1.0
    want = np.sum(sas, axis=1)[12] / 4
    want = want + 0.5 * ((np.arange(25) == 7) - want)
    assert np.array_equal(T[:, 12], np.broadcast_to(want, (n, 25)))
