"""The PMA calls — ``cobel_pma_store``, ``cobel_pma_replay``, ``cobel_pma_trial`` and
``cobel_pma_update_sr`` with its LDS kernel and its blocked kernels — with every table of the
memory inside a frame of sentinels (tests/frames_common.py): guards intact, the framed run
bit-equal to the plain run, the form told by the plans (and, for ``update_sr``, by the state count
and the switch that forces the blocked kernels), the work done asserted on the device results.

``update_sr`` runs on two instances: a tile of instance 0 that oversteps lands in instance 1's
block, where no guard sees it — the equality with the plain run, and with the LDS kernel's
result where both kernels serve the size, does."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
import pma_common as pc
import pma_wide_common as pw
from conftest import SEED

pytestmark = pytest.mark.gpu

POISON = {'rewards': fc.BIG, 'states': 0, 'terminals': 1, 'T': fc.BIG, 'SR': fc.BIG,
          'update_mask': 1}
WORLDS = {'5x5': (pc.demo_world, False), '6x7': (lambda: pc.seeded_world(6, 7, seed=8), False),
          '12x11': (pw.world_132, True)}


def _lib():
    from cobel_amd import _lib
    return _lib


def memory(world, n, wide, gamma=0.9):
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma=gamma, gamma_q=0.99, wide=wide)
    mem.bind(n, seed=SEED, instance_base=3)
    return mem


def swap_memory(frames, mem, length=32):
    for name in mem._dev:
        frames.swap(mem._dev, name, POISON[name])
    frames.swap(mem, 'counter', fc.MARK)
    mem._policy_counter()
    frames.swap(mem.policy, 'counter', fc.MARK)
    pows = mem._power_tables(length)
    mem._pows = (mem._pows[0], frames.add('gamma_pow', pows, fc.BIG))


def store(mem, frames, exp):
    """``PMAMemory.store`` with the experiences the test hands in framed."""
    from cobel_amd.memory import _device
    from cobel_amd.memory.pma import RECORD
    L = _lib()
    S = mem.nb_states
    rec = _device.records(exp, mem.n_envs, RECORD, {'state': S, 'action': mem.nb_actions,
                                                    'next_state': S}, none_as=-1)
    x = torch.as_tensor(rec.view(np.uint8), device=mem.device)
    if frames is not None:
        x = frames.add('experiences', x, 0)
    m = mem._mem()
    L.check(L.lib().cobel_pma_store(C.byref(m), L.ptr(x), L.current_stream(mem.device)))


def fill(mem, frames, tabs, stores=40):
    """A seeded walk of stores; instance i sees the walk i experiences late, so the tables differ;
    every instance ends with one experience at the LAST state."""
    rows = pc.walk_stores(tabs, stores, seed=3)
    n, S = mem.n_envs, mem.nb_states
    for k in range(len(rows)):
        pick = [rows[max(k - i, 0)] for i in range(n)]
        store(mem, frames, {'state': [r[0] for r in pick], 'action': [r[1] for r in pick],
                            'reward': [r[2] for r in pick], 'next_state': [r[3] for r in pick],
                            'terminal': [r[4] for r in pick]})
    nxt = int(tabs['next'][S - 1, 0])
    store(mem, frames, {'state': S - 1, 'action': 0, 'reward': 0.25, 'next_state': nxt,
                        'terminal': 1})


def tables(mem):
    out = {k: v.clone() for k, v in mem._dev.items()}
    out['counter'] = mem.counter.clone()
    out['pol_counter'] = mem.policy.counter.clone()
    return out


@pytest.mark.parametrize('n', [1, 9])
@pytest.mark.parametrize('name', list(WORLDS))
def test_pma_store_and_replay(name, n):
    """Stores, then replays of 1, 7 and 32 rounds from a given state, masked and not, with
    ``q[N][S][A]``, the records, the states and the mask framed: narrow form at 25 and 42 states,
    wide form at 132."""
    L = _lib()
    make, wide = WORLDS[name]
    world = make()
    tabs, _ = pc.tables_of(world)
    S, A = np.asarray(tabs['next']).shape
    start = int(tabs['starts'][0])
    mask = pc.masked_actions(tabs)
    outs = []
    for framed in (False, True):
        mem = memory(world, n, wide)
        frames = fc.Frames() if framed else None
        if framed:
            swap_memory(frames, mem)
        plan = mem.launch_plan(32)
        assert plan[1] == 64 and 0 < plan[0] <= 160 * 1024
        fill(mem, frames, tabs)
        out = {}
        q = torch.zeros((n, S, A), dtype=torch.float64, device=mem.device)
        bits = mem._mask_bits(mask)
        if framed:
            q = frames.add('q', q, fc.BIG)
            bits = frames.add('action_mask', bits, (1 << A) - 1)
        for length, masked in ((1, False), (7, True), (32, False)):
            st = torch.full((n,), start, dtype=torch.int32, device=mem.device)
            st[-1] = S - 1
            rec = torch.zeros((n, length * 24), dtype=torch.uint8, device=mem.device)
            if framed:
                st, rec = frames.add('current_state', st, 0), frames.add('records', rec, 0x5A)
            m = mem._mem(q, bits if masked else None, length)
            L.check(L.lib().cobel_pma_replay(C.byref(m), length, L.ptr(st), None, None, L.ptr(rec),
                                             L.current_stream(mem.device)))
            out['records_%d' % length] = rec.clone()
        torch.cuda.synchronize()
        if framed:
            frames.check()
        out['q'] = q.clone()
        out.update(tables(mem))
        outs.append(out)
        assert bool(q[-1].any()) and bool(q[0].any()), 'the replays changed no Q value'
        assert float(mem._dev['rewards'][-1, S - 1, 0].item()) != 0.0, 'nothing stored at the last state'
        assert int(mem._dev['states'][-1, S - 1, 0].item()) == int(tabs['next'][S - 1, 0])
    fc.assert_same(*outs)


def _sr_kernel(S):
    """'blocked' or 'lds': what ``cobel_pma_update_sr`` takes for ``S`` states as things stand (the
    switch that forces the blocked kernels included), read from the library: the wide plan reports
    the LDS of an update_sr workgroup by the same decision, and the blocked kernels' is one figure,
    that of 272 states.  (The narrow and the wide form of store / replay / trial are the memory's
    ``wide`` flag in ``cobel_pma_mem_t.flags``: the caller's choice, nothing the library decides.)"""
    from cobel_amd.memory import _device
    L = _lib()
    lds = lambda states: int(_device.plan4(L.lib().cobel_pma_plan_wide, states, 4, 0)[2])
    return 'blocked' if lds(S) == lds(272) else 'lds'


@pytest.mark.parametrize('kernel,world', [('lds', '5x5'), ('blocked', '5x5'), ('blocked', '12x11'),
                                          ('blocked', '17x16')])
def test_pma_update_sr(kernel, world, monkeypatch):
    """SR = inv(I - gamma T) on two instances, the float64 T and SR blocks of both framed: the LDS
    kernel at 25 states; the blocked kernels at 25 (less than one panel of 32 pivots, forced), at
    132 (four panels + 4, two tiles of 64 + 4) and at 272."""
    L = _lib()
    make, wide = {'17x16': (pw.world_272, True)}.get(world) or WORLDS[world]
    w = make()
    tabs, _ = pc.tables_of(w)
    S = int(np.asarray(tabs['next']).shape[0])
    forced = kernel == 'blocked' and S <= L.PMA_MAX_STATES
    outs = []
    for framed in (False, True):
        mem = memory(w, 2, wide)
        frames = fc.Frames() if framed else None
        if framed:
            swap_memory(frames, mem)
        fill(mem, frames, tabs)
        before = mem._dev['SR'].clone()
        if forced:
            monkeypatch.setenv('COBEL_DEBUG', '1')
            monkeypatch.setenv('COBEL_DEBUG_PMA_SR', 'blocked')
        try:
            mem.update_sr()
            torch.cuda.synchronize()
            assert _sr_kernel(S) == kernel
        finally:
            if forced:
                monkeypatch.delenv('COBEL_DEBUG_PMA_SR')
                monkeypatch.delenv('COBEL_DEBUG')
        if framed:
            frames.check()
        outs.append(tables(mem))
        sr = mem._dev['SR']
        assert bool(torch.isfinite(sr).all()) and not torch.equal(sr[0], sr[1])
        assert not torch.equal(sr[1, -1], before[1, -1]), 'the last row of the last instance is as before'
    fc.assert_same(*outs)
    # at 25 states both kernels serve, and the other one gives the same bits
    if S <= L.PMA_MAX_STATES:
        mem = memory(w, 2, wide)
        fill(mem, None, tabs)
        if not forced:
            monkeypatch.setenv('COBEL_DEBUG', '1')
            monkeypatch.setenv('COBEL_DEBUG_PMA_SR', 'blocked')
        mem.update_sr()
        torch.cuda.synchronize()
        assert torch.equal(mem._dev['SR'], outs[1]['SR'])
    # ... and the inverse it is, within the bound tests/pma_wide_common.py derives
    T, SR = outs[1]['T'].cpu().numpy(), outs[1]['SR'].cpu().numpy()
    for i in range(2):
        err = np.abs(SR[i] - np.linalg.inv(np.eye(S) - 0.9 * T[i])).max()
        assert err <= pw.sr_bound(S, 0.9), (i, err)


@pytest.mark.parametrize('n', [1, 9])
@pytest.mark.parametrize('name', list(WORLDS))
def test_pma_trial(name, n):
    """cobel_pma_trial, four trials of one launch each with ``update_sr`` in between, monitors of
    two trials only: Q, ``last``, the start-of-trial replay records, ``inst`` and the monitors
    framed beside the memory's tables."""
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.policy import EpsilonGreedy
    L = _lib()
    from cobel_amd.misc.gridworld_tools import make_gridworld
    h, w = [int(x) for x in name.split('x')]
    wide = WORLDS[name][1]
    S = h * w
    # (the one start is the LAST state, next to a rewarded state that ends no trial)
    world = make_gridworld(h, w, terminals=[S // 2], goals=[S // 2], starting_states=[S - 1],
                           rewards=np.array([[S // 2, 1.0], [S - 2, 0.25], [1, -0.5]]))
    tabs, _ = pc.tables_of(world)
    batch, steps, trial_cap, trials = 8, 30, 2, 4
    outs = []
    for framed in (False, True):
        from cobel_amd.memory import PMAMemory
        env = Gridworld(world, n_envs=n, seed=SEED, instance_base=3)
        mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, wide=wide)
        ag = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.3), mem)
        ag.track_instances = ag.track_occupancy = ag.track_responses = True
        ag.mask_actions, ag.action_mask = True, pc.masked_actions(tabs)
        ag._bind(env)
        ag._env_in(env)
        pol = ag.policy
        flags = L.F_LEARN | L.F_MASK_ACTIONS | ag._policy_in(pol, env, False)
        mem._session(env.seed, env.instance_base)
        ag.monitors.reserve(trial_cap, n, True)
        ag._mask_dev = ag._mask_bits()
        ag._start_records = torch.zeros((n, batch * 24), dtype=torch.uint8, device=ag.device)
        frames = fc.Frames() if framed else None
        if framed:
            fc.swap_fused(frames, ag)
            frames.swap(ag, '_q', fc.BIG)
            frames.swap(ag, '_last', 0)
            frames.swap(ag, '_start_records', 0x5A)
            frames.swap(ag, '_mask_dev', (1 << ag.n_actions) - 1)
            swap_memory(frames, mem, batch)
        plan = mem.launch_plan(batch)
        assert plan[1] == 64 and 0 < plan[0] <= 160 * 1024
        for t in range(trials):
            ag._launch(env, pol, flags, t + 1, steps, 0, batch)
            mem.update_sr()
        torch.cuda.synchronize()
        if framed:
            frames.check()
        out = {'q': ag._q.clone(), 'inst': ag.inst.clone(), 'last': ag._last.clone(),
               'start_records': ag._start_records.clone()}
        out.update(tables(mem))
        out.update({k: v.clone() for k, v in fc.monitor_arrays(ag.monitors).items()})
        outs.append(out)
        assert (ag.inst[:, L.I_TRIAL] == trials).all() and trials > trial_cap
        assert bool(ag._q[-1].any()), 'Q of the last instance did not change'
        assert bool(ag._q[:, -1].any()), 'the last row of Q changed in no instance'
        assert int(ag.monitors.steps_done.item()) > 0
    fc.assert_same(*outs)
