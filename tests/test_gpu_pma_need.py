"""``cobel_pma_stationary`` (csrc/pma_need.hip) on the device, and ``PMAMemory`` / ``PMA`` with
``offline_need = 'device'``.

Kernel: bit for bit the NumPy restatement ``pma_need_common.stationary_ref`` on every case of the
fixture — five instances holding the five tables of a world, with and without a selection, inside
sentinel frames, and one instance alone — and the degenerate rule.  Replay and training: the
``'device'`` mode against the ``'host'`` mode with ``compute_need`` replaced by a function that
returns the kernel's own vectors: identical bits go in, so identical bits must come out, whatever
near-ties ``gain * need`` holds.  Host reads: a ``'device'`` session reads nothing per trial."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
import pma_common as pc
import pma_need_common as nc
from conftest import SEED

pytestmark = pytest.mark.gpu

NEED_FILL, STATUS_FILL = -7.0, 77
SELECT = [-1, 3, -1, -1, 0]


def _lib():
    from cobel_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def Z(golden):
    return golden('pma_need')


@pytest.fixture(scope='module')
def restated(Z):
    """world -> (T [5, S, S], vectors [5, S], status [5]) of the restatement, computed once."""
    out = {}
    for world in nc.WORLDS:
        T = np.stack([Z[nc.case_name(world, n) + '/T'] for n in nc.STORES])
        sol = [nc.stationary_ref(t) for t in T]
        out[world] = (T, np.stack([s[0] for s in sol]), np.array([s[1] for s in sol]))
    return out


def call(T, select, frames):
    """``cobel_pma_stationary`` on the tables ``T`` [N, S, S] (device), ``need`` and ``status``
    pre-filled with sentinels: (need [N, S], status [N]) as NumPy."""
    L = _lib()
    n, S = T.shape[0], T.shape[1]
    need = torch.full((n, S), NEED_FILL, dtype=torch.float64, device=T.device)
    status = torch.full((n,), STATUS_FILL, dtype=torch.int32, device=T.device)
    sel = None if select is None else torch.tensor(select, dtype=torch.int32, device=T.device)
    if frames is not None:
        T = frames.add('T', T, fc.BIG)
        need = frames.add('need', need, fc.BIG)
        status = frames.add('status', status, fc.MARK)
        if sel is not None:
            sel = frames.add('select', sel, 0)       # (a stray read selects nothing)
    m = L.PMAMem()
    m.T, m.n, m.n_states, m.n_actions = L.ptr(T), n, S, 4
    L.check(L.lib().cobel_pma_stationary(C.byref(m), L.ptr(sel), L.ptr(need), L.ptr(status),
                                         L.current_stream(T.device)))
    torch.cuda.synchronize()
    if frames is not None:
        frames.check()
    return need.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize('world', list(nc.WORLDS))
def test_kernel_equals_the_restatement(restated, world):
    T, want, want_status = restated[world]
    assert (want_status == 0).all()
    dev = torch.device('cuda', torch.cuda.current_device())
    Td = torch.as_tensor(T, device=dev)
    need, status = call(Td, None, fc.Frames())
    for i, n in enumerate(nc.STORES):
        assert np.array_equal(need[i], want[i]), (world, n, np.abs(need[i] - want[i]).max())
    assert np.array_equal(status, want_status)
    plain, plain_status = call(Td, None, None)
    assert np.array_equal(plain, need) and np.array_equal(plain_status, status)
    # a selection: the skipped rows keep their fill
    part, part_status = call(Td, SELECT, fc.Frames())
    for i, s in enumerate(SELECT):
        if s < 0:
            assert np.array_equal(part[i], want[i]) and part_status[i] == 0
        else:
            assert (part[i] == NEED_FILL).all() and part_status[i] == STATUS_FILL
    # one instance alone gives what it gives inside the batch
    alone, alone_status = call(Td[2:3].contiguous(), None, fc.Frames())
    assert np.array_equal(alone[0], need[2]) and alone_status[0] == 0


def test_degenerate_ring_and_its_neighbour():
    """Instance 0: the ring with two absorbing states (status 1, the uniform row); instance 1: a
    regular chain of the same size, untouched by its neighbour's fate."""
    ring = nc.ring_two_absorbing()
    other = 0.5 * np.eye(6) + 0.3 * np.roll(np.eye(6), 1, axis=1) + 0.2 * np.roll(np.eye(6), -1, axis=1)
    other[0] = [0.1, 0.9, 0, 0, 0, 0]
    want, want_status = nc.stationary_ref(other)
    assert want_status == 0 and nc.stationary_ref(ring)[1] == 1
    dev = torch.device('cuda', torch.cuda.current_device())
    need, status = call(torch.as_tensor(np.stack([ring, other]), device=dev), None, fc.Frames())
    assert status.tolist() == [1, 0]
    assert np.array_equal(need[0], np.full(6, 1.0 / np.sqrt(6.0)))
    assert np.array_equal(need[1], want)


# -- PMAMemory ---------------------------------------------------------------------------------------
def filled_memory(n, mode, stores=60, seed=11):
    """demo_5x5 after ``walk_stores(tabs, stores, seed)``; instance i sees the walk i experiences
    late, so the tables differ."""
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = pc.demo_world()
    tabs, _ = pc.tables_of(world)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99)
    mem.bind(n, seed=SEED, instance_base=2)
    rows = pc.walk_stores(tabs, stores, seed=seed)
    for k in range(len(rows)):
        pick = [rows[max(k - i, 0)] for i in range(n)]
        mem.store({'state': [r[0] for r in pick], 'action': [r[1] for r in pick],
                   'reward': [r[2] for r in pick], 'next_state': [r[3] for r in pick],
                   'terminal': [r[4] for r in pick]})
    mem.update_sr()
    inject(mem, mode)
    return mem


def inject(mem, mode):
    """``'device'``, or ``'host'`` with ``compute_need`` returning the kernel's vectors."""
    if mode == 'device':
        mem.offline_need = 'device'
        return
    assert mem.offline_need == 'host'
    A = mem.nb_actions

    def compute_need(current_state=None, instances=None):
        assert current_state is None
        return np.tile(mem.stationary(instances).cpu().numpy(), (1, A))
    mem.compute_need = compute_need


def test_stationary_and_compute_need(Z):
    mem = filled_memory(3, 'device')
    T = mem.T
    want = np.stack([nc.stationary_ref(t)[0] for t in T])
    got = mem.stationary()
    assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)
    assert mem.need_status.dtype == torch.int32 and mem.need_status.tolist() == [0, 0, 0]
    assert np.array_equal(mem.stationary([2, 0]).cpu().numpy(), want[[2, 0]])
    need = mem.compute_need(None)
    assert isinstance(need, np.ndarray) and np.array_equal(need, np.tile(want, (1, 4)))
    assert np.array_equal(mem.compute_need(None, instances=[1]), np.tile(want[1:2], (1, 4)))
    # the host mode's vectors are close (a plausibility check, not an accuracy test: the eigenvalue
    # gap of these tables is down to 8e-6, and either solve errs by some 10 * 2^-53 / gap)
    mem.offline_need = 'host'
    assert np.abs(mem.compute_need(None) - need).max() < 1e-7


@pytest.mark.parametrize('states', [None, [None, 12, -1]], ids=['none', 'mixed'])
def test_replay_device_equals_host_with_the_same_vectors(states):
    n = 3
    q0 = np.random.default_rng(5).uniform(0, 1, (n, 25, 4))
    outs = []
    for mode in ('device', 'host'):
        mem = filled_memory(n, mode)
        ups, Q = mem.replay(q0, None, 7, states)
        outs.append({'ups': np.array([pc.rows_of(u) for u in ups]), 'Q': Q.cpu().numpy(),
                     'counter': mem.counter.cpu().numpy(),
                     'pol_counter': mem.policy.counter.cpu().numpy()})
        if mode == 'device':
            assert mem.need_status.tolist() == [0, 0, 0]
    assert outs[0]['ups'].shape == (n, 7, 5) and not np.array_equal(outs[0]['Q'], q0)
    assert (outs[0]['counter'] > 0).all()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


# -- PMA.train ---------------------------------------------------------------------------------------
PATH = [12, 17, 22, 23, 24, 19, 14, 9, 4]      # the shortest way of demo_5x5: eight steps


def session(mode, trials, n=4, spy=None):
    """``PMA.train(env, trials, 8, batch_size=4)`` on demo_5x5.  The shortest way from state 12
    takes all eight steps, so a learner that starts from nothing times out in every trial:
    instances 0 and 1 start with the values of that way in Q and arrive in about half of their
    trials, instances 2 and 3 start from zero."""
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = pc.demo_world()
    tabs, _ = pc.tables_of(world)
    nxt = np.asarray(tabs['next']).astype(int)
    env = Gridworld(world, n_envs=n, seed=SEED)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99)
    ag = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    ag._bind(env)
    q = np.zeros((n, 25, 4))
    for k in range(8):
        q[:2, PATH[k], int(np.flatnonzero(nxt[PATH[k]] == PATH[k + 1])[0])] = 10 * 0.99 ** (7 - k)
    ag.Q = torch.as_tensor(q)
    inject(mem, mode)
    if spy is not None:
        inner = mem._need_device

        def need_device(select):
            spy.append(select.clone())
            return inner(select)
        mem._need_device = need_device
    ag.train(env, trials, 8, batch_size=4)
    torch.cuda.synchronize()
    return ag, mem


def test_train_device_equals_host_with_the_same_vectors():
    lasts = []
    dev, dmem = session('device', 6, spy=lasts)
    host, hmem = session('host', 6)
    last = torch.stack(lasts).cpu().numpy()
    assert last.shape == (6, 4)
    assert (last == -1).any() and (last >= 0).any(), last
    assert (last == -1).sum() > (last >= 0).sum()          # (most trials time out)
    for name in ('T', 'SR', 'rewards', 'states', 'terminals'):
        assert torch.equal(dmem._dev[name], hmem._dev[name]), name
    assert torch.equal(dev._q, host._q) and torch.equal(dev.inst, host.inst)
    assert torch.equal(dmem.counter, hmem.counter)
    assert torch.equal(dmem.policy.counter, hmem.policy.counter)
    assert torch.equal(dev._last, host._last)
    assert dmem.need_status.tolist() == [0, 0, 0, 0]
    # the sessions did something: the walks reached T everywhere, the updates Q where it held values
    # (instances 2 and 3 never meet the reward: their Q stays zero)
    fresh = torch.as_tensor(pc.RefPMAMemory(pc.tables_of(pc.demo_world())[1], None).T,
                            device=dev.device)
    assert all(not torch.equal(dmem._dev['T'][i], fresh) for i in range(4))
    assert float((dev._q[:2] != 0).sum()) > 16, 'the replays and steps changed no other Q value'


def test_device_session_reads_nothing_per_trial(monkeypatch):
    """Calls of ``Tensor.cpu`` / ``.item`` / ``.tolist`` in a session without callbacks: as many
    for nine trials as for three with ``'device'``; with ``'host'`` every trial adds some."""
    count = [0]
    for name in ('cpu', 'item', 'tolist'):
        inner = getattr(torch.Tensor, name)

        def counted(self, *args, _inner=inner, **kwargs):
            count[0] += 1
            return _inner(self, *args, **kwargs)
        monkeypatch.setattr(torch.Tensor, name, counted)
    reads = {}
    for mode in ('device', 'host'):
        for trials in (3, 9):
            count[0] = 0
            session(mode, trials)
            reads[mode, trials] = count[0]
    assert reads['device', 3] == reads['device', 9], reads
    assert reads['host', 9] > reads['host', 3], reads
