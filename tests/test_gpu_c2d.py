"""The continuous 2D arena on the device against the float64 restatement of tests/c2d_common.py:
the step robot bit for bit (state, reward, done, wall, counters after every step, for every lane
mapping), resets, sharding, the wheel robot within the bound derived below, and a DQN run whose
every stored transition the restatement reproduces."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c2d_common as cc  # noqa: E402

pytestmark = pytest.mark.gpu
LANES = (0, 1, 4, 16, 64)       # 0: the planner's choice


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch


class Arena:
    """Device tables of one geometry and framed outputs for ``n`` instances."""

    def __init__(self, torch, T, R, n, S=None, box=None, fallback=None, robot=cc.STEP, seed=0xC2D,
                 base=0, lanes=0, **params):
        from cobel_amd import _lib
        self.torch, self._lib, self.n = torch, _lib, n
        S = T if S is None else S
        self.edges = torch.as_tensor(T, device='cuda').contiguous()
        self.spawn = torch.as_tensor(S, device='cuda').contiguous()
        self.rewards = torch.as_tensor(np.ascontiguousarray(R), device='cuda') if len(R) else None
        self.state, c1 = cc.framed(torch, (n, 3), torch.float64, -7.5)
        self.ctr, c2 = cc.framed(torch, (n,), torch.int32, -3)
        self.reward, c3 = cc.framed(torch, (n,), torch.float64, -7.5)
        self.done, c4 = cc.framed(torch, (n,), torch.uint8, 99)
        self.wall, c5 = cc.framed(torch, (n,), torch.uint8, 99)
        self.fallbacks, c6 = cc.framed(torch, (1,), torch.int32, -3)
        self.state.zero_(), self.ctr.zero_(), self.fallbacks.zero_()
        self.frames = (c1, c2, c3, c4, c5, c6)
        box = cc.bounds(T) if box is None else box
        fallback = cc.first_grid_point(T, S, box)[0] if fallback is None else fallback
        self.c = cc.fill(_lib, _lib.ptr(self.edges), _lib.ptr(self.spawn), _lib.ptr(self.rewards),
                         _lib.ptr(self.state), _lib.ptr(self.ctr), n, T.shape[1], S.shape[1], len(R), box,
                         fallback, robot=robot, seed=seed, base=base, lanes=lanes, **params)

    def step(self, actions):
        act = self.torch.as_tensor(np.ascontiguousarray(actions, dtype=np.uint8), device='cuda')
        self._lib.check(self._lib.lib().cobel_c2d_step(
            C.byref(self.c), self._lib.ptr(act), self._lib.ptr(self.reward), self._lib.ptr(self.done),
            self._lib.ptr(self.wall), None))

    def reset(self, mask=None):
        m = None if mask is None else self.torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8),
                                                           device='cuda')
        self._lib.check(self._lib.lib().cobel_c2d_reset(C.byref(self.c), self._lib.ptr(m),
                                                        self._lib.ptr(self.fallbacks), None))

    def put(self, state):
        self.state.copy_(self.torch.as_tensor(np.ascontiguousarray(state), device='cuda'))

    def get(self):
        """state, reward, done, wall, counters — after a synchronisation, frames checked."""
        out = [t.cpu().numpy() for t in (self.state, self.reward, self.done, self.wall)]
        out.append(self.ctr.cpu().numpy().view(np.uint32))
        for check in self.frames:
            check()
        return out


def _same(got, want, what):
    assert got.dtype == want.dtype and np.array_equal(got, want), \
        (what, np.argwhere(got != want)[:4].tolist())


# -- the step robot, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 64, 65, 300])
@pytest.mark.parametrize('name', ['square', 'open_field', 'eight', 'ring1024'])
def test_step_robot_matches_the_restatement(torch_cuda, name, n):
    """E = 4, 75, 12 (with holes) and 1 024; starts planted within 0.02 of the walls, actions held
    for runs of steps and a few the robot does not have; punish_wall on; the open field's two
    reward rows overlap (the first wins), the square has none.  After the initial reset and after
    every one of 40 steps (a masked reset follows step 20) everything is compared with
    np.array_equal, for every lane mapping."""
    W = cc.walk(name)
    hits = sum(int(r[3][:n].sum()) for r in W.records)
    assert n < 64 or hits >= n, hits                    # the cases do run into walls
    for lanes in LANES:
        A = Arena(torch_cuda, W.T, W.R, n, seed=W.seed, lanes=lanes, **W.params)
        A.reset()
        state, _, _, _, ctr = A.get()
        _same(state, W.after_reset[0][:n], 'first reset: state')
        _same(ctr, W.after_reset[1][:n], 'first reset: counters')
        A.put(W.start[:n])
        for t, (state, reward, done, wall, ctr) in enumerate(W.records):
            A.step(W.actions[t, :n])
            if t == W.reset_at:
                A.reset(W.mask[:n])
            got = A.get()
            for g, w, what in zip(got, (state, reward, done, wall, ctr),
                                  ('state', 'reward', 'done', 'wall', 'counters')):
                _same(g, w[:n], (what, 'step', t, 'lanes', lanes))
        assert int(A.fallbacks.item()) == 0


def test_cases_cover_rewards_overlap_and_strays():
    """What the seeded cases contain, on the restatement alone (so that a pass above means
    something): trial ends, the first of two overlapping rows paying where the second is in reach
    too, wall punishments, actions the robot does not have."""
    W = cc.walk('open_field')
    done = np.stack([r[2] for r in W.records])
    reward = np.stack([r[1] for r in W.records])
    states = np.stack([r[0] for r in W.records])
    keep = np.arange(W.steps) != W.reset_at              # (there the states are the reset's)
    done, reward, states = done[keep], reward[keep], states[keep]
    first = np.hypot(states[..., 0] - 0.75, states[..., 1] - 0.75) <= 0.1
    second = np.hypot(states[..., 0] - 0.78, states[..., 1] - 0.75) <= 0.1
    strayed = W.actions[keep] >= 4
    assert (first & second & (done == 1)).sum() >= 10 and (reward[first & ~strayed] == 10.0).all()
    assert (~first & second & (done == 1)).sum() >= 3 and (reward[~first & second & ~strayed] == 5.0).all()
    assert sum(int(r[2].sum()) for r in cc.walk('eight').records) >= 10
    assert (reward == -10.0).sum() >= 300 and (W.actions >= 4).sum() >= 100
    assert (cc.walk('square').R.shape == (0, 3)) and not np.stack([r[2] for r in cc.walk('square').records]).any()


def test_punish_wall_off(torch_cuda):
    W = cc.walk('open_field', punish=0)
    assert not any((r[1] == -10.0).any() for r in W.records) and sum(int(r[3].sum()) for r in W.records) > 300
    n = 65
    for lanes in (0, 1, 16):
        A = Arena(torch_cuda, W.T, W.R, n, seed=W.seed, lanes=lanes, **W.params)
        A.put(W.start[:n])
        A.ctr.copy_(torch_cuda.as_tensor(W.after_reset[1][:n].view(np.int32), device='cuda'))
        for t, want in enumerate(W.records):
            A.step(W.actions[t, :n])
            if t == W.reset_at:
                A.reset(W.mask[:n])
            for g, w in zip(A.get(), want):
                _same(g, w[:n], ('step', t, 'lanes', lanes))


def test_hand_cases_and_refusal(torch_cuda):
    """The hand cases of the host test on the device, for every lane mapping; 1 025 edges are
    refused."""
    from cobel_amd import _lib
    sq, wedge = cc.table(cc.UNIT_SQUARE), cc.table(cc.WEDGE)
    none = np.zeros((0, 3))
    for lanes in LANES:
        A = Arena(torch_cuda, sq, none, 2, lanes=lanes)
        A.put([[0.5, 0.01, 0.0], [0.5, 0.5, 0.0]])
        A.step([3, 0])
        state, reward, done, wall, _ = A.get()
        assert state.tolist() == [[0.5, 1e-6, 0.0], [0.485, 0.5, 0.0]]
        assert (reward.tolist(), done.tolist(), wall.tolist()) == ([0.0, 0.0], [0, 0], [1, 0])
        A = Arena(torch_cuda, wedge, none, 1, lanes=lanes, fallback=(0.5, 0.0), punish_wall=1)
        A.put([[3.5e-5, 0.0, 0.0]])
        A.step([1])
        state, reward, done, wall, _ = A.get()
        assert state.tolist() == [[3.5e-5, 0.0, 0.0]]
        assert (reward.tolist(), done.tolist(), wall.tolist()) == ([-10.0], [0], [1])
    big = cc.table(cc.gon(0.5, 0.5, 0.5, 1025))
    A = Arena(torch_cuda, big[:, :1024], none, 1, fallback=(0.5, 0.5))
    A.c.n_edges = 1025
    with pytest.raises(IndexError, match='1025 edges'):
        A.step([0])
    out = (C.c_int32 * 4)()
    assert _lib.lib().cobel_c2d_plan(1, 1025, C.byref(out)) == _lib.E_RANGE


# -- reset -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('robot', [cc.STEP, cc.WHEEL])
def test_reset_masks_candidates_and_counters(torch_cuda, robot):
    """A diamond spawn that fills half of its box: the first accepted candidate in counter order,
    counters + 2 k* + 4, orientation 2 pi u (0 for the step robot), unmasked instances unchanged to
    the bit; twice in a row; for every lane mapping."""
    T, R = cc.geometries()['open_field']
    S = cc.table([(0.5, 0.1), (0.9, 0.5), (0.5, 0.9), (0.1, 0.5)])
    box, fallback, seed, n, base = np.array([0.1, 0.1, 0.9, 0.9]), (0.5, 0.3), 4242, 65, 1000
    rng = np.random.default_rng(8)
    state0 = rng.random((n, 3))
    ctr0 = (2 * rng.integers(0, 50, n)).astype(np.uint32)
    ctr0[3] = 0xFFFFFFFE                                  # the counter wraps
    masks = [(rng.random(n) < 0.6).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8), None]
    want_s, want_c, later = state0.copy(), ctr0.copy(), 0
    wants = []
    for mask in masks:
        for i in range(n):
            if mask is None or mask[i]:
                want_s[i], want_c[i], fell, k = cc.reset(T, S, box, fallback, robot, seed, base + i,
                                                         int(want_c[i]))
                later += int(k > 0)
                assert not fell
        wants.append((want_s.copy(), want_c.copy()))
    assert later >= 20
    for lanes in LANES:
        A = Arena(torch_cuda, T, R, n, S=S, box=box, fallback=fallback, robot=robot, seed=seed, base=base,
                  lanes=lanes)
        A.put(state0)
        A.ctr.copy_(torch_cuda.as_tensor(ctr0.view(np.int32), device='cuda'))
        for mask, (ws, wc) in zip(masks, wants):
            A.reset(mask)
            state, _, _, _, ctr = A.get()
            _same(state, ws, ('state', lanes))      # (2 pi u is one multiplication: exact)
            _same(ctr, wc, ('counters', lanes))
        assert int(A.fallbacks.item()) == 0
        if robot == cc.STEP:
            assert not state[:, 2].any()


def test_reset_falls_back_after_1024_candidates(torch_cuda):
    """A spawn table that no candidate of the box can satisfy: the fallback point, the orientation
    from draw c + 2048, counters + 2052, the device counter incremented once per instance."""
    T, R = cc.geometries()['square']
    S = cc.table([(5.0, 5.0), (6.0, 5.0), (6.0, 6.0), (5.0, 6.0)])
    n, seed, fallback = 5, 31, (0.25, 0.75)
    for lanes, robot in ((0, cc.WHEEL), (1, cc.STEP), (64, cc.WHEEL)):
        A = Arena(torch_cuda, T, R, n, S=S, box=cc.bounds(T), fallback=fallback, robot=robot, seed=seed,
                  lanes=lanes)
        A.ctr.fill_(6)
        mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
        A.reset(mask)
        state, _, _, _, ctr = A.get()
        for i in range(n):
            if mask[i]:
                ws, wc, fell, _ = cc.reset(T, S, cc.bounds(T), fallback, robot, seed, i, 6)
                assert fell and wc == 6 + 2052
                assert state[i].tolist() == list(ws) and ctr[i] == wc
            else:
                assert state[i].tolist() == [0.0, 0.0, 0.0] and ctr[i] == 6
        assert int(A.fallbacks.item()) == 3


def test_sharding(torch_cuda):
    """128 instances in one launch equal two launches of 64 with instance_base 0 and 64."""
    W = cc.walk('open_field')
    whole = Arena(torch_cuda, W.T, W.R, 128, seed=W.seed, **W.params)
    parts = [Arena(torch_cuda, W.T, W.R, 64, seed=W.seed, base=b, **W.params) for b in (0, 64)]
    for A in [whole] + parts:
        A.reset()
    for t in range(12):
        whole.step(W.actions[t, :128])
        for k, A in enumerate(parts):
            A.step(W.actions[t, 64 * k:64 * k + 64])
        if t == 5:
            whole.reset(W.mask[:128])
            for k, A in enumerate(parts):
                A.reset(W.mask[64 * k:64 * k + 64])
        got = whole.get()
        halves = [A.get() for A in parts]
        for j, g in enumerate(got):
            _same(g, np.concatenate([halves[0][j], halves[1][j]]), ('step', t, j))
    assert not np.array_equal(halves[0][0], halves[1][0])       # (the halves drew different starts)


# -- the wheel robot ---------------------------------------------------------------------------------------
def test_wheel_robot_within_the_derived_bound(torch_cuda):
    """The device's sin and cos differ from libm's in the last bits, so positions cannot be bit
    equal; the orientation must be (2 theta mod 2 pi and theta' = theta are exact).  One step at a
    time from the restatement's own state, uploaded each step: flags, rewards and orientations
    bit-equal, positions within 1e-13.

    Derivation of the bound: a free step errs by at most step_size x a few ulp of sin / cos plus one
    rounding of the sum, about 2.3e-16; a hit multiplies that by at most 1 / sin(phi), about 10 at
    the admitted incidence phi >= 0.1 rad; the rest is margin.  tests/test_host_c2d.py asserts on
    the restatement alone that every hit of these cases has phi >= 0.1 rad and that every discrete
    decision clears its threshold by >= 1e-9.  The mappings must agree with each other to the bit."""
    W = cc.wheel_walk()
    outs = {}
    worst = 0.0
    for lanes in LANES:
        A = Arena(torch_cuda, W.T, W.R, W.n, robot=cc.WHEEL, lanes=lanes, **W.params)
        outs[lanes] = []
        for t in range(W.steps):
            A.put(W.before[t])
            A.step(W.actions[t])
            state, reward, done, wall, _ = A.get()
            ws, wr, wd, ww = W.after[t]
            _same(reward, wr, ('reward', t, lanes))
            _same(done, wd, ('done', t, lanes))
            _same(wall, ww, ('wall', t, lanes))
            _same(state[:, 2], ws[:, 2], ('theta', t, lanes))
            err = float(np.abs(state[:, :2] - ws[:, :2]).max())
            worst = max(worst, err)
            outs[lanes].append(state)
        for t in range(W.steps):
            _same(outs[lanes][t], outs[LANES[0]][t], ('mappings differ', t, lanes))
    print('wheel robot: largest position difference %.3e' % worst)
    assert worst <= 1e-13, worst


# -- the class ---------------------------------------------------------------------------------------------
def _demo_arena():
    from cobel_amd.misc import continuous_tools as ct
    room = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    obstacles = [ct.make_rectangle(np.ones(2) / 2, 0.1, 0.1, 45), ct.make_circle(np.array([0.9, 0.1]), 0.05),
                 ct.make_triangle(np.array([0.1, 0.9]), 0.1, 0.1)]
    return room, None, obstacles, np.array([[0.75, 0.75, 10.0]])


def test_interface_scalar_and_vector_forms(torch_cuda):
    torch = torch_cuda
    from cobel_amd.interface import Continuous2D
    env = Continuous2D('step', *_demo_arena(), seed=5)
    T, g = env.geometry['edges'], env.geometry
    ws, wc, _, _ = cc.reset(T, g['spawn_edges'], g['box'], g['fallback'], cc.STEP, 5, 0, 0)
    assert env.state[0].tolist() == list(ws) and int(env.env_ctr[0]) == wc and env.reset_fallbacks == 0
    env.step_size, env.punish_wall = 0.02, True            # read at every call
    p = dict(cc.DEFAULTS, step_size=0.02, punish_wall=1)
    state = ws
    for t, a in enumerate([0, 0, 1, 3, 2, 2]):
        obs, reward, end, truncated, logs = env.step(a)
        state, wr, wd, ww = cc.step(T, env.R, cc.STEP, state, a, p)
        assert isinstance(obs, np.ndarray) and obs.tolist() == list(state[:2]) and logs == {}
        assert (reward, end, truncated, env.wall_hit) == (wr, bool(wd), bool(wd), bool(ww))
        assert type(reward) is float and type(end) is bool and env.current_step == t + 1
    assert env.get_position().tolist() == list(state[:2])
    env.R = np.array([[state[0], state[1], 3.5]])           # an edit of R goes out with the next call
    assert env.step(0)[1:3] == (3.5, True)
    obs, logs = env.reset()
    assert obs.shape == (2,) and logs == {} and env.current_step == 0 and int(env.env_ctr[0]) % 2 == 0
    with pytest.raises(AssertionError, match='Invalid action'):
        env.step(4)

    env = Continuous2D('wheel', *_demo_arena(), n_envs=70, seed=6, instance_base=10)
    before = env.state.cpu().numpy()
    assert env.observe().shape == (70, 3) and (before[:, 2] > 0).all()
    act = torch.randint(0, 3, (70,), device='cuda')
    obs, reward, done, truncated, logs = env.step(act)
    assert torch.is_tensor(obs) and obs.shape == (70, 3) and reward.dtype == torch.float64
    assert done.dtype == torch.bool and done is truncated and env._done.dtype == torch.uint8
    for i in (0, 33, 69):
        ws, wr, wd, ww = cc.step(T, env.R, cc.WHEEL, before[i], int(act[i]))
        assert np.allclose(obs[i].cpu().numpy(), ws, atol=1e-13) and float(reward[i]) == wr
    frozen = env.state.clone()
    mask = torch.arange(70, device='cuda') % 2 == 0
    env.reset(mask)
    assert torch.equal(env.state[1::2], frozen[1::2]) and not torch.equal(env.state[0::2], frozen[0::2])
    assert env.get_position().shape == (70, 2)
    for lanes in (1, 4, 16, 64):                             # the attribute reaches the launch
        env.lanes_per_instance = lanes
        env.step(act)
    env.lanes_per_instance = 3
    with pytest.raises(AssertionError, match='3 lanes per instance'):
        env.step(act)


def test_dqn_end_to_end(torch_cuda):
    """DQN with the demo's tanh 64-64 network in float64 on four instances of the open field, two
    trials of at most 20 steps: the run completes, the monitors hold two trials, and every stored
    transition (state, action -> next_state, reward, non-terminal flag) is one restatement step."""
    torch = torch_cuda
    from cobel_amd.agent import DQN
    from cobel_amd.interface import Continuous2D
    from cobel_amd.network import TorchNetwork
    from cobel_amd.policy import EpsilonGreedy

    class Model(torch.nn.Module):
        def __init__(self, n_in, n_out):
            super().__init__()
            self.layer_dense_1 = torch.nn.Linear(n_in, 64)
            self.layer_dense_2 = torch.nn.Linear(64, 64)
            self.layer_output = torch.nn.Linear(64, n_out)
            self.double()

        def forward(self, x):
            x = torch.tanh(self.layer_dense_1(x))
            x = torch.tanh(self.layer_dense_2(x))
            return self.layer_output(x)

    torch.manual_seed(0)
    env = Continuous2D('step', *_demo_arena(), n_envs=4, seed=17)
    agent = DQN(env.observation_space, env.action_space, EpsilonGreedy(0.1), TorchNetwork(Model(2, 4)),
                0.9 ** 0.15)
    agent.train(env, 2, 20, batch_size=8)
    torch.cuda.synchronize()
    assert agent.trial.tolist() == [2, 2, 2, 2]
    assert agent.monitors.raw('lat_cnt').sum(dim=0).tolist()[:3] == [4, 4] + [0] * (agent.monitors.cap > 2)
    assert np.isfinite(agent.monitors.mean_latency()[:2]).all()
    M = agent.M
    size = M.size.cpu().numpy()
    assert (size >= 2).all() and (M.head.cpu().numpy() == 0).all()
    s, a, r = M.states.cpu().numpy(), M.actions.cpu().numpy(), M.rewards.cpu().numpy()
    ns, nt = M.next_states.cpu().numpy(), M.terminals.cpu().numpy()
    T, checked = env.geometry['edges'], 0
    for i in range(4):
        for k in range(size[i]):
            ws, wr, wd, _ = cc.step(T, env.R, cc.STEP, (s[i, k, 0], s[i, k, 1], 0.0), int(a[i, k]))
            assert ns[i, k].tolist() == list(ws[:2]) and r[i, k] == wr and nt[i, k] == 1.0 - wd, (i, k)
            checked += 1
    assert checked >= 40
