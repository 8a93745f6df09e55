"""``cobel_pma_stationary_wide`` (csrc/pma_need_wide.hip) on the device, and ``PMAMemory(wide=True,
need_workspace=k)`` / ``PMA`` with ``offline_need = 'device'``.

Kernels: bit for bit the NumPy restatement ``pma_need_common.stationary_ref`` — the contract of the
LDS kernel, unchanged — on the fixture worlds of 129 .. 1 024 states, on general matrices that swap
rows at nearly every step across every panel and tile edge, on small sizes (where
``cobel_pma_stationary`` must give the same bits), for every grouping the workspace imposes, and on
degenerate inputs.  Replay and training: the ``'device'`` mode against the ``'host'`` mode with
``compute_need`` replaced by a function that returns the kernels' own vectors.  Host reads: a wide
``'device'`` session reads nothing per trial."""
import ctypes as C

import numpy as np
import pytest
import torch

import frames_common as fc
import pma_common as pc
import pma_need_common as nc
import pma_need_wide_common as wc
from conftest import SEED

pytestmark = pytest.mark.gpu

NEED_FILL, STATUS_FILL = -7.0, 77


def _lib():
    from cobel_amd import _lib
    return _lib


def device():
    return torch.device('cuda', torch.cuda.current_device())


@pytest.fixture(scope='module')
def Z(golden):
    return golden('pma_need_wide')


@pytest.fixture(scope='module')
def restated(Z):
    """world -> (T [3, S, S], vectors [3, S], status [3]) of the restatement, computed once."""
    out = {}
    for world in wc.MID_WORLDS:
        T = np.stack([Z[wc.case_name(world, n) + '/T'] for n in wc.STORES])
        out[world] = (T,) + restate(T)
    return out


def restate(T):
    sol = [nc.stationary_ref(t) for t in T]
    return np.stack([s[0] for s in sol]), np.array([s[1] for s in sol])


def call(T, select=None, frames=None, held=None, entry='wide'):
    """``cobel_pma_stationary_wide`` on the tables ``T`` [N, S, S] (NumPy or device) with a workspace
    for ``held`` instances (default: all), ``need`` and ``status`` pre-filled with sentinels: (need
    [N, S], status [N]) as NumPy.  ``entry='lds'``: ``cobel_pma_stationary``."""
    L = _lib()
    T = torch.as_tensor(np.ascontiguousarray(T), device=device()) if not torch.is_tensor(T) else T
    n, S = T.shape[0], T.shape[1]
    need = torch.full((n, S), NEED_FILL, dtype=torch.float64, device=T.device)
    status = torch.full((n,), STATUS_FILL, dtype=torch.int32, device=T.device)
    sel = None if select is None else torch.tensor(select, dtype=torch.int32, device=T.device)
    per = wc.work_bytes(S)
    work = torch.full(((held or n) * per // 8,), fc.BIG, dtype=torch.float64, device=T.device)
    if frames is not None:
        T = frames.add('T', T, fc.BIG)
        need = frames.add('need', need, fc.BIG)
        status = frames.add('status', status, fc.MARK)
        work = frames.add('work', work, fc.BIG)
        if sel is not None:
            sel = frames.add('select', sel, 0)       # (a stray read selects nothing)
    m = L.PMAMem()
    m.T, m.n, m.n_states, m.n_actions = L.ptr(T), n, S, 4
    if entry == 'wide':
        L.check(L.lib().cobel_pma_stationary_wide(
            C.byref(m), L.ptr(sel), L.ptr(need), L.ptr(status), L.ptr(work), work.numel() * 8,
            L.current_stream(T.device)))
    else:
        L.check(L.lib().cobel_pma_stationary(C.byref(m), L.ptr(sel), L.ptr(need), L.ptr(status),
                                             L.current_stream(T.device)))
    torch.cuda.synchronize()
    if frames is not None:
        frames.check()
    return need.cpu().numpy(), status.cpu().numpy()


def assert_rows(need, status, want, want_status, what):
    for i in range(len(want)):
        assert np.array_equal(need[i], want[i]), (what, i, np.abs(need[i] - want[i]).max())
    assert np.array_equal(status, want_status), (what, status)


@pytest.mark.parametrize('world', list(wc.MID_WORLDS))
def test_kernels_equal_the_restatement(restated, world):
    T, want, want_status = restated[world]
    assert T.shape[1] == wc.STATES[world] and (want_status == 0).all()
    Td = torch.as_tensor(T, device=device())
    need, status = call(Td, None, fc.Frames())
    assert_rows(need, status, want, want_status, world)
    plain, plain_status = call(Td)
    assert np.array_equal(plain, need) and np.array_equal(plain_status, status)
    # a selection: the skipped row keeps its fill
    part, part_status = call(Td, [-1, 5, -1], fc.Frames())
    for i in (0, 2):
        assert np.array_equal(part[i], want[i]) and part_status[i] == 0
    assert (part[1] == NEED_FILL).all() and part_status[1] == STATUS_FILL
    # one instance alone gives what it gives inside the batch
    alone, alone_status = call(Td[2:3].contiguous(), None, fc.Frames())
    assert np.array_equal(alone[0], need[2]) and alone_status[0] == 0


@pytest.mark.parametrize('S', wc.GENERAL_SIZES)
def test_pivoting_on_general_matrices(S):
    """``normal`` and ``dyadic``: a swap at more than 90 % of the steps, partners farther away than
    any panel or tile is wide, and exactly tied pivot columns in ``dyadic``."""
    T = np.stack([wc.normal(S), wc.dyadic(S)])
    stats = [wc.elimination_stats(t) for t in T]
    for st in stats:
        assert st['zero_at'] is None and st['swaps'] > 0.9 * S and st['reach'] > 100, st
    assert stats[0]['ties'] == 0 and 3 <= stats[1]['ties'] <= 5, stats
    want, want_status = restate(T)
    assert (want_status == 0).all()
    need, status = call(T, None, fc.Frames())
    assert_rows(need, status, want, want_status, S)


SMALL_FIXTURE = {12: 'small_3x4', 128: 'seeded_8x16'}


@pytest.mark.parametrize('S', [1, 2, 12, 33, 64, 65, 128])
def test_small_sizes_and_the_lds_kernel(golden, S):
    """Below the wide form's own range the entry point serves all the same, and
    ``cobel_pma_stationary`` gives the same bits on the same tables."""
    tables = [wc.dyadic(S)]
    if S in SMALL_FIXTURE:
        Zs = golden('pma_need')
        tables += [Zs[nc.case_name(SMALL_FIXTURE[S], n) + '/T'] for n in nc.STORES]
    T = np.stack(tables)
    if S >= 12:
        st = wc.elimination_stats(T[0])
        assert st['swaps'] >= 0.75 * S and st['ties'] >= 1, st
    want, want_status = restate(T)
    assert (want_status == 0).all()
    need, status = call(T, None, fc.Frames())
    assert_rows(need, status, want, want_status, S)
    lds, lds_status = call(T, None, fc.Frames(), entry='lds')
    assert np.array_equal(lds, need) and np.array_equal(lds_status, status)


def test_the_result_does_not_depend_on_the_group_size(restated):
    S = 150
    T = np.concatenate([restated['seeded_10x15'][0], wc.normal(S)[None], wc.dyadic(S)[None]])
    want, want_status = restate(T)
    outs = [call(T, None, fc.Frames(), held=held) for held in (5, 2, 1)]
    assert_rows(outs[0][0], outs[0][1], want, want_status, 'five')
    for need, status in outs[1:]:
        assert np.array_equal(need, outs[0][0]) and np.array_equal(status, outs[0][1])
    # with a selection, a group whose instances are all skipped included
    need, status = call(T, [0, 0, -1, 3, -1], fc.Frames(), held=2)
    for i in range(5):
        if i in (2, 4):
            assert np.array_equal(need[i], want[i]) and status[i] == 0
        else:
            assert (need[i] == NEED_FILL).all() and status[i] == STATUS_FILL


# where the first exactly zero pivot falls (step k, counted from 0): the identity gives 1 / S
# everywhere, so every row equals the first; a ring of m states besides S - m absorbing ones loses
# the pivot at step m + 1 (searched on the CPU: m = 70 puts it at step 71, the eighth of the fifth
# panel of sixteen)
DEGENERATE = {
    'identity_150': (lambda: np.eye(150), 1),
    'ring_148_of_150': (lambda: wc.ring_absorbing(150, 148), 149),
    'ring_219_of_221': (lambda: wc.ring_absorbing(221, 219), 220),
    'ring_254_of_256': (lambda: wc.ring_absorbing(256, 254), 255),
    'ring_70_of_150': (lambda: wc.ring_absorbing(150, 70), 71),
}


@pytest.mark.parametrize('name', list(DEGENERATE))
def test_degenerate_between_two_regular_instances(name):
    build, zero_at = DEGENERATE[name]
    bad = build()
    S = bad.shape[0]
    assert wc.elimination_stats(bad)['zero_at'] == zero_at
    assert 0 < zero_at % wc.PANEL or name != 'ring_70_of_150'
    T = np.stack([wc.regular(S, 1), bad, wc.regular(S, 2)])
    want, want_status = restate(T)
    assert want_status.tolist() == [0, 1, 0]
    need, status = call(T, None, fc.Frames())
    assert status.tolist() == [0, 1, 0]
    assert np.array_equal(need[1], np.full(S, 1.0 / np.sqrt(float(S))))
    assert np.array_equal(need[0], want[0]) and np.array_equal(need[2], want[2])
    # the workspace of a degenerate instance serves the next group as any other
    need, status = call(T, None, fc.Frames(), held=1)
    assert status.tolist() == [0, 1, 0] and np.array_equal(need, np.stack(want))


def test_1024_states_with_a_workspace_for_one():
    T = np.stack([wc.case_T(wc.BIG, n) for n in wc.BIG_STORES])
    assert T.shape == (2, 1024, 1024)
    want, want_status = restate(T)
    assert (want_status == 0).all()
    need, status = call(T, None, fc.Frames(), held=1)
    assert_rows(need, status, want, want_status, wc.BIG)


# -- PMAMemory ---------------------------------------------------------------------------------------
WORLD = 'seeded_10x15'


def filled_memory(n, mode, stores=60, seed=11):
    """The 150-state world after ``walk_stores(tabs, stores, seed)``; instance i sees the walk i
    experiences late, so the tables differ."""
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = wc.WORLDS[WORLD]()
    tabs, _ = pc.tables_of(world)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, wide=True, need_workspace=2)
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
    """``'device'``, or ``'host'`` with ``compute_need`` returning the kernels' vectors."""
    if mode == 'device':
        mem.offline_need = 'device'
        return
    assert mem.offline_need == 'host'
    A = mem.nb_actions

    def compute_need(current_state=None, instances=None):
        assert current_state is None
        return np.tile(mem.stationary(instances).cpu().numpy(), (1, A))
    mem.compute_need = compute_need


def test_stationary_and_compute_need():
    mem = filled_memory(3, 'device')
    assert mem._need_work.numel() == 2 * wc.work_bytes(150)      # (for two of three instances)
    T = mem.T
    want = np.stack([nc.stationary_ref(t)[0] for t in T])
    assert not np.array_equal(want[0], want[2])
    got = mem.stationary()
    assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)
    assert mem.need_status.dtype == torch.int32 and mem.need_status.tolist() == [0, 0, 0]
    assert np.array_equal(mem.stationary([2, 0]).cpu().numpy(), want[[2, 0]])
    need = mem.compute_need(None)
    assert isinstance(need, np.ndarray) and np.array_equal(need, np.tile(want, (1, 4)))
    assert np.array_equal(mem.compute_need(None, instances=[1]), np.tile(want[1:2], (1, 4)))
    # the host mode's vectors are close (a plausibility check, not an accuracy test)
    mem.offline_need = 'host'
    assert np.abs(mem.compute_need(None) - need).max() < 1e-7


def test_the_workspace_is_clipped_to_the_instance_count():
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = wc.WORLDS[WORLD]()
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), wide=True, need_workspace=64)
    mem.bind(2, seed=SEED)
    assert mem._need_work.numel() == 2 * wc.work_bytes(150)
    want = nc.stationary_ref(np.asarray(mem.T)[0])[0]
    assert np.array_equal(mem.stationary().cpu().numpy(), np.stack([want, want]))
    # without a workspace the wide form has no device path
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), wide=True)
    mem.bind(2, seed=SEED)
    assert mem._need_work is None
    with pytest.raises(NotImplementedError, match='need_workspace'):
        mem.stationary()


@pytest.mark.parametrize('states', [None, [None, 75, -1]], ids=['none', 'mixed'])
def test_replay_device_equals_host_with_the_same_vectors(states):
    n = 3
    q0 = np.random.default_rng(5).uniform(0, 1, (n, 150, 4))
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
def way_values(tabs):
    """Q [S, A] = 10 * 0.99 ** (steps from the successor to the terminal state): a learner that
    starts with them walks the shortest way from anywhere.  Also the length of that way from the
    starting state."""
    nxt = np.asarray(tabs['next']).astype(int)
    term = np.asarray(tabs['terminal']).astype(bool)
    S, A = nxt.shape
    dist = np.full(S, -1)
    dist[term] = 0
    todo = [int(s) for s in np.flatnonzero(term)]
    while todo:
        u = todo.pop(0)
        for s, a in zip(*np.nonzero(nxt == u)):
            if dist[s] < 0:
                dist[s] = dist[u] + 1
                todo.append(int(s))
    assert (dist >= 0).all()
    return 10 * 0.99 ** dist[nxt], int(dist[int(tabs['starts'][0])])


def session(mode, trials, n=4, spy=None):
    """``PMA.train(env, trials, way + 20, batch_size=4)`` on the 150-state world.  Instance 0 starts
    with the values of the shortest ways in Q and arrives (the replays of a memory that has seen
    nothing yet undo some of those values around the start, which costs it up to fifteen steps more
    in the first trial); the others start from nothing and time out."""
    from cobel_amd.agent import PMA
    from cobel_amd.interface import Gridworld
    from cobel_amd.memory import PMAMemory
    from cobel_amd.policy import EpsilonGreedy
    world = wc.WORLDS[WORLD]()
    tabs, _ = pc.tables_of(world)
    values, way = way_values(tabs)
    assert way >= 8
    env = Gridworld(world, n_envs=n, seed=SEED)
    mem = PMAMemory(world['sas'], EpsilonGreedy(0.1), gamma_q=0.99, wide=True, need_workspace=2)
    ag = PMA(env.observation_space, env.action_space, EpsilonGreedy(0.1), mem)
    ag._bind(env)
    q = np.zeros((n, 150, 4))
    q[0] = values
    ag.Q = torch.as_tensor(q)
    inject(mem, mode)
    if spy is not None:
        inner = mem._need_device

        def need_device(select):
            spy.append(select.clone())
            return inner(select)
        mem._need_device = need_device
    ag.train(env, trials, way + 20, batch_size=4)
    torch.cuda.synchronize()
    return ag, mem


def test_train_device_equals_host_with_the_same_vectors():
    lasts = []
    dev, dmem = session('device', 5, spy=lasts)
    host, hmem = session('host', 5)
    last = torch.stack(lasts).cpu().numpy()
    assert last.shape == (5, 4)
    assert (last == -1).any() and (last >= 0).any(), last
    assert (last == -1).sum() > (last >= 0).sum()          # (most trials time out)
    for name in ('T', 'SR', 'rewards', 'states', 'terminals'):
        assert torch.equal(dmem._dev[name], hmem._dev[name]), name
    assert torch.equal(dev._q, host._q) and torch.equal(dev.inst, host.inst)
    assert torch.equal(dmem.counter, hmem.counter)
    assert torch.equal(dmem.policy.counter, hmem.policy.counter)
    assert torch.equal(dev._last, host._last)
    assert dmem.need_status.tolist() == [0, 0, 0, 0]
    fresh = torch.as_tensor(pc.RefPMAMemory(pc.tables_of(wc.WORLDS[WORLD]())[1], None).T,
                            device=dev.device)
    assert all(not torch.equal(dmem._dev['T'][i], fresh) for i in range(4))


def test_device_session_reads_nothing_per_trial(monkeypatch):
    """Calls of ``Tensor.cpu`` / ``.item`` / ``.tolist`` in a session without callbacks: as many
    for six trials as for two with ``'device'``; with ``'host'`` every trial adds some."""
    count = [0]
    for name in ('cpu', 'item', 'tolist'):
        inner = getattr(torch.Tensor, name)

        def counted(self, *args, _inner=inner, **kwargs):
            count[0] += 1
            return _inner(self, *args, **kwargs)
        monkeypatch.setattr(torch.Tensor, name, counted)
    reads = {}
    for mode in ('device', 'host'):
        for trials in (2, 6):
            count[0] = 0
            session(mode, trials)
            reads[mode, trials] = count[0]
    assert reads['device', 2] == reads['device', 6], reads
    assert reads['host', 6] > reads['host', 2], reads
