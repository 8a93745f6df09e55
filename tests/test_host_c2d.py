"""Host side of the continuous 2D arena: the restatement's hand cases and invariant, the templates,
the geometry build and its refusals, the reset's bookkeeping, the conditions the wheel cases of the
GPU test rest on, and the agreement of header, ctypes and library on the new exports."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c2d_common as cc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cobel_c2d_plan', 'cobel_c2d_step', 'cobel_c2d_reset')
OUT_OF_SCOPE = 'general polygon clipping is out of scope'


# -- the restatement ----------------------------------------------------------------------------------
def test_hand_cases_on_the_unit_square():
    T = cc.table(cc.UNIT_SQUARE)
    assert T.shape == (8, 4)
    state, reward, done, wall = cc.step(T, np.zeros((0, 3)), cc.STEP, (0.5, 0.01, 0.0), 3)
    assert state == (0.5, 1e-6, 0.0) and (reward, done, wall) == (0.0, 0, 1)
    state, reward, done, wall = cc.step(T, np.zeros((0, 3)), cc.STEP, (0.5, 0.5, 0.0), 0)
    assert state == (0.485, 0.5, 0.0) and (reward, done, wall) == (0.0, 0, 0)
    # punish_wall, and a reward row in reach wins over the punishment; the first row in reach pays
    p = dict(cc.DEFAULTS, punish_wall=1)
    assert cc.step(T, np.zeros((0, 3)), cc.STEP, (0.5, 0.01, 0.0), 3, p)[1:] == (-10.0, 0, 1)
    R = np.array([[0.9, 0.9, 3.0], [0.5, 0.05, 7.0], [0.5, 0.0, 9.0]])
    assert cc.step(T, R, cc.STEP, (0.5, 0.01, 0.0), 3, p)[1:] == (7.0, 1, 1)
    # an action the robot does not have
    assert cc.step(T, R, cc.STEP, (0.5, 0.01, 0.0), 4, p) == ((0.5, 0.01, 0.0), 0.0, 0, 0)
    assert cc.step(T, R, cc.WHEEL, (0.5, 0.5, 1.0), 3, p) == ((0.5, 0.5, 1.0), 0.0, 0, 0)


def test_hand_case_the_guard_refuses_in_a_wedge():
    """Triangle (0, 0) (1, -0.0175) (1, 0.0175): from (3.5e-5, 0) "up" hits the upper side, the
    point pushed m inwards from there is nearer than m / 2 to the lower side or outside, and the
    robot stays."""
    T = cc.table(cc.WEDGE)
    assert cc.clear(T, 3.5e-5, 0.0)
    diag = {}
    x, y, hit = cc.move(T, 3.5e-5, 0.0, 3.5e-5, 0.015, cc.M, diag)
    assert (x, y, hit) == (3.5e-5, 0.0, True) and diag['guard'] and 'phi' in diag
    assert cc.step(T, np.zeros((0, 3)), cc.STEP, (3.5e-5, 0.0, 0.0), 1) == ((3.5e-5, 0.0, 0.0), 0.0, 0, 1)


def test_wheel_arithmetic_keeps_the_reference_s_quirks():
    p = cc.DEFAULTS
    th = 0.7
    tx, ty, th2 = cc.target_of(cc.WHEEL, 0.3, 0.4, th, 2, p)
    assert (tx, ty, th2) == (0.3 + math.cos(th) * 0.015, 0.4 + math.sin(th) * 0.015, th)
    for a, R in ((0, 0.05), (1, -0.05)):
        tx, ty, th2 = cc.target_of(cc.WHEEL, 0.3, 0.4, th, a, p)
        om = (0.15, -0.15)[a]
        icc = (0.3 - R * math.sin(th), 0.4 + R * math.sin(th))       # (both with the sine)
        rel = (0.3 - icc[0], 0.4 - icc[1])
        assert tx == pytest.approx(math.cos(om) * rel[0] - math.sin(om) * rel[1] + icc[0], abs=1e-15)
        assert ty == pytest.approx(math.sin(om) * rel[0] + math.cos(om) * rel[1] + icc[1], abs=1e-15)
        assert th2 == th + th                                           # (theta, not omega, is added)
    assert cc.target_of(cc.WHEEL, 0.3, 0.4, 4.0, 0, p)[2] == math.fmod(8.0, cc.TWO_PI)
    assert cc.py_mod(-1.0, cc.TWO_PI) == -1.0 + cc.TWO_PI and cc.py_mod(cc.TWO_PI, cc.TWO_PI) == 0.0


@pytest.mark.parametrize('robot', [cc.STEP, cc.WHEEL])
def test_invariant_clear_after_every_step(robot):
    """40 walks of 250 steps on the demo's open field: a robot that is clear stays clear, and a
    healthy share of the steps runs into a wall."""
    T, R = cc.geometries()['open_field']
    rng = np.random.default_rng(5 + robot)
    box, hits, refused = cc.bounds(T), 0, 0
    fallback, accepted = cc.first_grid_point(T, T, box)
    assert accepted >= 256
    for w in range(40):
        state, _, fell, _ = cc.reset(T, T, box, fallback, robot, 77, w, 0)
        assert not fell and cc.clear(T, state[0], state[1])
        actions = cc.held_actions(1, 250, 4 if robot == cc.STEP else 3, rng, stray=0.0)[:, 0]
        for a in actions:
            diag = {}
            x, y, th = state
            tx, ty, th2 = cc.target_of(robot, x, y, th, int(a), cc.DEFAULTS)
            cx, cy, hit = cc.move(T, x, y, tx, ty, cc.M, diag)
            assert cc.clear(T, cx, cy), (w, state, int(a))
            assert 0.0 <= th2 < cc.TWO_PI
            hits, refused = hits + int(hit), refused + int(diag['guard'])
            state = (cx, cy, th2)
    assert 500 <= hits <= 5000, hits
    assert refused <= 20, refused


def test_wheel_cases_meet_their_conditions():
    """What the position bound of the GPU test (1e-13) rests on, asserted on the restatement alone:
    every hit has an incidence of at least 0.1 rad and every discrete decision (hit or no hit and
    which edge, guard, reward radius) is at least 1e-9 from its threshold.  A seed that fails is to
    be changed, not the bound."""
    W = cc.wheel_walk()
    hits = 0
    for t in range(W.steps):
        for i in range(W.n):
            d = W.diags[t][i]
            if not d:       # not an action of the robot
                assert W.actions[t, i] >= 3
                continue
            assert d['margin'] >= 1e-9, (t, i, d)
            if 'phi' in d:
                hits += 1
                assert d['phi'] >= 0.1, (t, i, d)
    assert hits >= 40, hits
    walls = sum(int(a[3].sum()) for a in W.after)
    assert walls >= 40 and sum(int(a[2].sum()) for a in W.after) >= 10      # ... and rewards are reached


# -- templates ------------------------------------------------------------------------------------------
def _open(poly_ring):
    c = np.asarray(poly_ring.coords)
    assert np.array_equal(c[0], c[-1])
    return c[:-1]


def test_templates_match_hand_worked_vertices():
    from cobel_amd.misc import continuous_tools as ct
    room, spawn, obstacles, rewards = ct.make_t_maze(2.0, 1.0, 0.5, 'right', 10)
    assert _open(room.exterior).tolist() == [[0, 2.5], [2.5, 2.5], [2.5, 2], [1.5, 2], [1.5, 0], [1, 0],
                                             [1, 2], [0, 2]]
    assert _open(spawn.exterior).tolist() == [[1, 0], [1.5, 0], [1.5, 0.5], [1, 0.5]]
    assert obstacles == [] and rewards.tolist() == [[2.25, 2.25, 10]]
    assert ct.make_t_maze(2.0, 1.0, 0.5, 'left')[3].tolist() == [[0.25, 2.25, 1]]
    assert ct.make_t_maze(2.0, 1.0, 0.5, 'none')[3].size == 0
    assert room.bounds == (0.0, 0.0, 2.5, 2.5) and room.interiors == []

    room, spawn, _, rewards = ct.make_double_t_maze(2.0, 2.0, 0.5, 'right-right', 3)
    assert _open(room.exterior).tolist() == [
        [0, 4.5], [3.5, 4.5], [3.5, 4], [2, 4], [2, 2.5], [5.5, 2.5], [5.5, 4], [4, 4], [4, 4.5],
        [7.5, 4.5], [7.5, 4], [6, 4], [6, 2], [4, 2], [4, 0], [3.5, 0], [3.5, 2], [1.5, 2], [1.5, 4],
        [0, 4]]
    assert _open(spawn.exterior).tolist() == [[3.5, 0], [4, 0], [4, 0.5], [3.5, 0.5]]
    assert rewards.tolist() == [[7.25, 4.25, 3]]
    assert ct.make_double_t_maze(2.0, 2.0, 0.5, 'left-right')[3].tolist() == [[3.25, 4.25, 1]]

    room, spawn, _, rewards = ct.make_two_sided_t_maze(2.0, 1.0, 0.5, 'right-right', 2)
    assert _open(room.exterior).tolist() == [
        [0, 2.5], [0.5, 2.5], [0.5, 1.5], [2.5, 1.5], [2.5, 2.5], [3, 2.5], [3, 0], [2.5, 0],
        [2.5, 1], [0.5, 1], [0.5, 0], [0, 0]]
    assert _open(spawn.exterior).tolist() == [[1.25, 1], [1.75, 1], [1.75, 1.5], [1.25, 1.5]]
    assert rewards.tolist() == [[2.75, 0.25, 2]]
    assert ct.make_two_sided_t_maze(2.0, 1.0, 0.5, 'left-right')[3].tolist() == [[0.25, 2.25, 1]]

    room, spawn, _, rewards = ct.make_eight_maze(2.0, 1.0, 0.5, 'right', 4)
    assert _open(room.exterior).tolist() == [[0, 0], [3.5, 0], [3.5, 3], [0, 3]]
    assert [_open(r).tolist() for r in room.interiors] == [
        [[0.5, 0.5], [1.5, 0.5], [1.5, 2.5], [0.5, 2.5]], [[2, 0.5], [3, 0.5], [3, 2.5], [2, 2.5]]]
    assert _open(spawn.exterior).tolist() == [[1.5, 1.25], [2, 1.25], [2, 1.75], [1.5, 1.75]]
    assert rewards.tolist() == [[3.25, 1.5, 4]]

    room, spawn, _, rewards = ct.make_cross_maze(1.0, 0.5, 'top', 6)
    assert _open(room.exterior).tolist() == [
        [-1.25, 0.25], [-0.25, 0.25], [-0.25, 1.25], [0.25, 1.25], [0.25, 0.25], [1.25, 0.25],
        [1.25, -0.25], [0.25, -0.25], [0.25, -1.25], [-0.25, -1.25], [-0.25, -0.25], [-1.25, -0.25]]
    assert _open(spawn.exterior).tolist() == [[-0.25, 0.25], [0.25, 0.25], [0.25, -0.25], [-0.25, -0.25]]
    assert rewards.tolist() == [[0, 1, 6]]
    room, _, _, rewards = ct.make_cross_maze(1.0, 0.5, 'right', 1, rotation=90.0)
    assert np.allclose(_open(room.exterior)[:3], [[-0.25, -1.25], [-0.25, -0.25], [-1.25, -0.25]], atol=1e-15)
    assert np.allclose(rewards, [[0, 1, 1]], atol=1e-15)


def test_obstacle_templates():
    from cobel_amd.misc import continuous_tools as ct
    assert _open(ct.make_rectangle(np.array([2.0, 1.0]), 2.0, 1.0).exterior).tolist() == [
        [1, 0.5], [3, 0.5], [3, 1.5], [1, 1.5]]
    d = 0.05 * math.sqrt(2.0)       # rotation about its own centre, then the translation
    assert np.allclose(_open(ct.make_rectangle(np.ones(2) / 2, 0.1, 0.1, 45).exterior),
                       [[0.5, 0.5 - d], [0.5 + d, 0.5], [0.5, 0.5 + d], [0.5 - d, 0.5]], atol=1e-15)
    h = 0.9 - 0.1 / 3.0             # the centroid goes to the location
    assert np.allclose(_open(ct.make_triangle(np.array([0.1, 0.9]), 0.1, 0.1).exterior),
                       [[0.05, h], [0.15, h], [0.1, h + 0.1]], atol=1e-15)
    # (0,0) (3,0) (0,3): centroid (1,1) to the origin, then 90 degrees about the box centre (.5,.5)
    assert np.allclose(_open(ct.make_triangle(np.zeros(2), 3.0, 3.0, 0.0, 90.0).exterior),
                       [[2, -1], [2, 2], [-1, -1]], atol=1e-14)
    c = _open(ct.make_circle(np.array([0.9, 0.1]), 0.05).exterior)
    assert c.shape == (64, 2) and c[0].tolist() == [0.9 + 0.05, 0.1]
    assert np.allclose(c[16], [0.9, 0.15], atol=1e-15) and cc.area2(c) > 0
    assert np.allclose(np.hypot(c[:, 0] - 0.9, c[:, 1] - 0.1), 0.05, atol=1e-15)
    assert 'not claimed' in ct.make_circle.__doc__


def test_demo_open_field_has_75_edges_and_matches_the_formulas():
    from cobel_amd.interface.continuous import build_geometry
    from cobel_amd.misc import continuous_tools as ct
    room = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])
    obstacles = [ct.make_rectangle(np.ones(2) / 2, 0.1, 0.1, 45), ct.make_circle(np.array([0.9, 0.1]), 0.05),
                 ct.make_triangle(np.array([0.1, 0.9]), 0.1, 0.1)]
    g = build_geometry(room, None, obstacles)
    T = cc.geometries()['open_field'][0]
    assert g['edges'].shape == (8, 75) == T.shape
    assert g['spawn_edges'] is g['edges'] and g['limits'].tolist() == [0, 0, 1, 1]
    # the same polygon up to the last digits of the obstacles' vertices and where each ring starts
    for probe in np.random.default_rng(3).random((400, 2)):
        assert cc.inside(g['edges'], *probe) == cc.inside(T, *probe)
    first, count = cc.first_grid_point(g['edges'], g['edges'], g['box'])
    assert g['fallback'].tolist() == list(first) and g['accepted'] == count >= 256


# -- geometry build -----------------------------------------------------------------------------------
def test_geometry_orientation_is_normalised():
    from cobel_amd.interface.continuous import build_geometry, clear, inside
    from cobel_amd.misc.continuous_tools import Polygon
    hole = [(0.4, 0.4), (0.6, 0.4), (0.6, 0.6), (0.4, 0.6)]
    want = cc.table(cc.UNIT_SQUARE, [hole])
    for room in (cc.UNIT_SQUARE, cc.UNIT_SQUARE[::-1]):
        for obstacle in (hole, hole[::-1]):
            T = build_geometry(room, None, [Polygon(obstacle)])['edges']
            assert sorted(T.T.tolist()) == sorted(want.T.tolist())
            mid = np.stack([T[0] + 0.5 * T[4] + 1e-5 * T[6], T[1] + 0.5 * T[5] + 1e-5 * T[7]], axis=1)
            assert inside(T, mid).all() and clear(T, mid, 1e-6).all()      # interior to the left
            assert not inside(T, np.array([[0.5, 0.5], [1.5, 0.5]])).any()
    # a room with a hole of its own (duck-typed: .exterior.coords / .interiors) equals room + obstacle
    T = build_geometry(Polygon(cc.UNIT_SQUARE, [hole]), None, None)['edges']
    assert np.array_equal(T, want)
    # the package's table is the formulas' table, bit for bit; a repeated vertex gives no edge
    doubled = [cc.UNIT_SQUARE[0]] + list(cc.UNIT_SQUARE)
    assert np.array_equal(build_geometry(doubled, None, [hole])['edges'], want)


def test_geometry_refusals():
    from cobel_amd.interface.continuous import build_geometry
    from cobel_amd.misc import continuous_tools as ct
    sq = cc.UNIT_SQUARE
    with pytest.raises(ValueError, match=OUT_OF_SCOPE):     # crosses the border
        build_geometry(sq, None, [ct.make_rectangle((0.95, 0.5), 0.2, 0.2)])
    with pytest.raises(ValueError, match=OUT_OF_SCOPE):     # touches the border
        build_geometry(sq, None, [ct.make_rectangle((0.9, 0.5), 0.2, 0.2)])
    with pytest.raises(ValueError, match=OUT_OF_SCOPE):     # outside
        build_geometry(sq, None, [ct.make_rectangle((2.0, 0.5), 0.2, 0.2)])
    with pytest.raises(ValueError, match=OUT_OF_SCOPE):     # two obstacles cross
        build_geometry(sq, None, [ct.make_rectangle((0.5, 0.5), 0.2, 0.2), ct.make_circle((0.6, 0.5), 0.1)])
    with pytest.raises(ValueError, match=OUT_OF_SCOPE):     # one inside the other
        build_geometry(sq, None, [ct.make_rectangle((0.5, 0.5), 0.4, 0.4), ct.make_circle((0.5, 0.5), 0.1)])
    with pytest.raises(ValueError, match=OUT_OF_SCOPE):     # inside a hole the room already has
        build_geometry(ct.make_eight_maze(2.0, 1.0, 0.5)[0], None, [ct.make_circle((1.0, 1.5), 0.1)])
    with pytest.raises(ValueError, match='1025 edges'):
        build_geometry(cc.gon(0.5, 0.5, 0.5, 1025), None, None)
    assert build_geometry(cc.gon(0.5, 0.5, 0.5, 1024), None, None)['edges'].shape == (8, 1024)


def test_spawn_region():
    from cobel_amd.interface.continuous import build_geometry
    from cobel_amd.misc import continuous_tools as ct
    sq = cc.UNIT_SQUARE
    with pytest.raises(ValueError, match='spawn area too thin for rejection sampling'):
        build_geometry(sq, ct.make_rectangle((0.5, 0.5), 1.2, 0.004, 45), None)
    g = build_geometry(sq, [(5, 5), (6, 5), (6, 6), (5, 6)], None)       # no overlap: the arena
    assert g['spawn_edges'] is g['edges'] and g['box'].tolist() == [0, 0, 1, 1]
    g = build_geometry(sq, [(0.5, 0.25), (1.5, 0.25), (1.5, 0.75), (0.5, 0.75)], None)
    assert g['box'].tolist() == [0.5, 0.25, 1.0, 0.75]                   # clipped to the arena
    assert np.array_equal(g['spawn_edges'], cc.table([(0.5, 0.25), (1.5, 0.25), (1.5, 0.75), (0.5, 0.75)]))
    first, count = cc.first_grid_point(g['edges'], g['spawn_edges'], g['box'])
    assert g['fallback'].tolist() == list(first) and g['accepted'] == count == 64 * 64
    room, spawn, _, _ = ct.make_eight_maze(0.4, 0.3, 0.1)
    g = build_geometry(room, spawn, None)
    assert g['edges'].shape == (8, 12) and g['spawn_edges'].shape == (8, 4)
    assert np.allclose(g['box'], [0.4, 0.25, 0.5, 0.35])


# -- reset ----------------------------------------------------------------------------------------------
def test_reset_takes_the_first_accepted_candidate_and_counts():
    T, _ = cc.geometries()['open_field']
    S = cc.table([(0.5, 0.1), (0.9, 0.5), (0.5, 0.9), (0.1, 0.5)])      # half of its box
    box, fallback, seed = np.array([0.1, 0.1, 0.9, 0.9]), (0.5, 0.3), 99
    later = 0
    for g in range(24):
        c = 0
        for robot in (cc.STEP, cc.WHEEL, cc.STEP):
            k = 0
            while True:
                qx = 0.1 + (0.9 - 0.1) * cc.draw(seed, g, c + 2 * k)
                qy = 0.1 + (0.9 - 0.1) * cc.draw(seed, g, c + 2 * k + 1)
                if cc.inside(S, qx, qy) and cc.clear(T, qx, qy):
                    break
                k += 1
            state, c2, fell, k_star = cc.reset(T, S, box, fallback, robot, seed, g, c)
            th = cc.TWO_PI * cc.draw(seed, g, c + 2 * k + 2)
            assert (k_star, fell, c2) == (k, False, c + 2 * k + 4) and c2 % 2 == 0
            assert state == (qx, qy, th if robot == cc.WHEEL else 0.0)
            later += k > 0
            c = c2
    assert later >= 10
    state, c2, fell, k_star = cc.reset(T, S, box, fallback, cc.WHEEL, seed, 3, 10, refuse_all=True)
    assert fell and k_star is None and c2 == 10 + 2052
    assert state == (0.5, 0.3, cc.TWO_PI * cc.draw(seed, 3, 10 + 2048))
    assert cc.reset(T, S, box, fallback, cc.STEP, seed, 3, 10, refuse_all=True)[0] == (0.5, 0.3, 0.0)
    # the draws are cobel_draw_u01's: counter c -> half c & 1 of block c >> 1
    from oracle import philox
    b = philox._block(seed, 3, 5, 0, philox.STREAM_ENV)
    assert cc.draw(seed, 3, 11) == ((int(b[2]) >> 5) * 67108864.0 + (int(b[3]) >> 6)) / 9007199254740992.0


# -- the class on the host ------------------------------------------------------------------------------
def test_interface_attributes_and_live_values():
    from cobel_amd import _lib
    from cobel_amd.interface import Continuous2D
    from cobel_amd.misc import continuous_tools as ct
    names = [p.name for p in inspect.signature(Continuous2D.__init__).parameters.values()][1:]
    assert names == ['robot_type', 'room', 'spawn', 'obstacles', 'rewards', 'simulator', 'widget', 'rng',
                     'n_envs', 'seed', 'device', 'instance_base']
    room, spawn, obstacles, rewards = ct.make_t_maze(0.4, 0.2, 0.1, reward=10)
    env = Continuous2D('step', room, spawn, obstacles, rewards, device='cpu', seed=4, n_envs=3)
    assert env.R is rewards and env.room is room and env.spawn is spawn and env.obstacles == []
    assert (env.buffer, env.punish_wall, env.type) == (-1e-6, False, 'step')
    assert (env.body_radius, env.wheel_radius, env.wheel_distance, env.step_size) == (0.05, 0.02, 0.1, 0.015)
    assert env.observation_space.shape == (2,) and int(env.action_space.n) == 4
    assert np.allclose(env.limits, [0, 0, 0.5, 0.5]) and env.current_step == 0
    assert env.state.shape == (3, 3) and env.observe().shape == (3, 2)
    assert env._reward.dtype.is_floating_point and env._reward.element_size() == 8
    assert env._done.element_size() == 1 and (env.seed, env.instance_base, env.n_envs) == (4, 0, 3)
    env.initialize_visualization(), env.update_visualization()
    wheel = Continuous2D('wheel', room, None, None, np.array([]), device='cpu', seed=4)
    assert wheel.observation_space.shape == (3,) and int(wheel.action_space.n) == 3
    assert wheel.observe().shape == (1, 3) and wheel.spawn is room and wheel.descriptor().n_rewards == 0
    with pytest.raises(AssertionError):
        Continuous2D('step', room, spawn, obstacles, rewards, simulator=object(), device='cpu')
    with pytest.raises(_lib.CobelHipError, match='built on the host'):
        env.step(np.zeros(3))
    with pytest.raises(_lib.CobelHipError, match='built on the host'):
        env.reset()
    # scalar attributes are read at every call; an edit of R goes out with sync_world()
    env.step_size, env.punish_wall = 0.02, True
    d = env.descriptor()
    assert (d.step_size, d.punish_wall, d.buffer, d.n, d.n_edges, d.n_spawn_edges, d.n_rewards) == \
        (0.02, 1, -1e-6, 3, 8, 4, 1)
    assert d.robot_type == _lib.C2D_STEP and d.lanes_per_instance == 0 and d.seed == 4
    assert not env.sync_world()
    env.R[0, 2] = 3.0
    assert env.sync_world() and not env.sync_world()
    assert env._R_dev[0].tolist() == [env.R[0, 0], env.R[0, 1], 3.0]
    env.R = np.zeros((33, 3))
    with pytest.raises(ValueError, match='33 reward rows'):
        env.sync_world()


# -- the library ------------------------------------------------------------------------------------------
def test_exports_header_and_struct_agree(tmp_path):
    from cobel_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cobel_hip.h')).read()
    lib = _lib.lib()
    assert lib.cobel_abi_version() == 1017
    for name in NEW:
        m = re.search(r'COBEL_API\s+int\s+%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert name in _lib.EXPORTS
        getattr(lib, name)
        assert len(m.group(1).split(',')) == len(_lib._SIGNATURES[name][1]), name
    assert re.search(r'#define COBEL_C2D_MAX_EDGES %d\b' % _lib.C2D_MAX_EDGES, header)
    assert re.search(r'#define COBEL_C2D_MAX_REWARDS %d\b' % _lib.C2D_MAX_REWARDS, header)
    assert re.search(r'#define COBEL_C2D_STEP %d\b' % _lib.C2D_STEP, header)
    assert re.search(r'#define COBEL_C2D_WHEEL %d\b' % _lib.C2D_WHEEL, header)
    assert (_lib.C2D_MAX_EDGES, _lib.C2D_MAX_REWARDS) == (1024, 32)
    assert (cc.STEP, cc.WHEEL) == (_lib.C2D_STEP, _lib.C2D_WHEEL)
    assert len(re.findall(r'continuous\.py:\d+', header)) >= 6       # the lines each call replaces
    cc_bin = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    assert cc_bin is not None, 'no C compiler'
    fields = [f for f, _ in _lib.C2D._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include "cobel_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(cobel_c2d_t));\n'
                   + ''.join('printf("%%zu\\n", offsetof(cobel_c2d_t, %s));\n' % f for f in fields)
                   + 'return 0; }\n')
    exe = tmp_path / 's'
    subprocess.check_call([cc_bin, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.C2D) == 160
    assert got[1:] == [getattr(_lib.C2D, f).offset for f in fields]
    assert (_lib.C2D.box.offset, _lib.C2D.seed.offset, _lib.C2D.instance_base.offset) == (40, 120, 156)


def test_planner():
    from cobel_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 4)()
    for n, E, want in ((1, 4, [4, 256, 256, 1]), (1, 75, [64, 256, 4800, 1]), (300, 75, [64, 256, 4800, 75]),
                       (1024, 75, [64, 256, 4800, 256]), (1025, 75, [16, 256, 4800, 65]),
                       (4096, 75, [16, 256, 4800, 256]), (16384, 75, [16, 256, 4800, 1024]),
                       (16385, 75, [4, 256, 4800, 257]), (65536, 75, [4, 256, 4800, 1024]),
                       (65537, 75, [1, 256, 4800, 257]), (65536, 2, [1, 256, 128, 256]),
                       (1 << 20, 75, [1, 256, 4800, 4096]), (5, 1, [1, 256, 64, 1]), (5, 3, [4, 256, 192, 1]),
                       (5, 5, [4, 256, 320, 1]), (5, 16, [16, 256, 1024, 1]), (5, 17, [16, 256, 1088, 1]),
                       (5, 33, [64, 256, 2112, 2]), (5, 1024, [64, 256, 65536, 2]), (0, 75, [64, 256, 4800, 0])):
        assert lib.cobel_c2d_plan(n, E, C.byref(out)) == _lib.OK
        assert list(out) == want, (n, E)
    assert lib.cobel_c2d_plan(1, 75, None) == _lib.E_ARG
    assert lib.cobel_c2d_plan(-1, 75, C.byref(out)) == _lib.E_RANGE
    assert lib.cobel_c2d_plan(1, 0, C.byref(out)) == _lib.E_RANGE
    assert lib.cobel_c2d_plan(1, 1025, C.byref(out)) == _lib.E_RANGE
    with pytest.raises(IndexError, match='1025 edges'):
        _lib.check(lib.cobel_c2d_plan(1, 1025, C.byref(out)))


def test_library_refuses_before_touching_the_device():
    """Every refusal of the three entry points comes back with its code on a host without a GPU:
    the checks run before any HIP call."""
    from cobel_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(64)
    p = _lib.ptr(buf)

    def arena(**kw):
        a = dict(edges=p, spawn_edges=p, rewards=p, state=p, env_ctr=p, n=1, n_edges=4, n_spawn=4,
                 n_rewards=1, box=(0, 0, 1, 1), fallback=(0.5, 0.5))
        a.update(kw)
        return cc.fill(_lib, **a)

    def step(c, action=p, reward=p, done=p, wall=p):
        return lib.cobel_c2d_step(C.byref(c) if c is not None else None, action, reward, done, wall, None)

    def reset(c, fallbacks=p):
        return lib.cobel_c2d_reset(C.byref(c) if c is not None else None, None, fallbacks, None)

    for call in (step, reset):
        assert call(None) == _lib.E_ARG
        for name in ('edges', 'spawn_edges', 'state', 'env_ctr', 'rewards'):
            assert call(arena(**{name: None})) == _lib.E_ARG, name
        assert call(arena(edges=p + 4)) == _lib.E_ARG and call(arena(env_ctr=p + 2)) == _lib.E_ARG
        for bad in (0, -1, 1025):
            assert call(arena(n_edges=bad)) == _lib.E_RANGE, bad
            assert call(arena(n_spawn=bad)) == _lib.E_RANGE, bad
        assert call(arena(n_rewards=33)) == _lib.E_RANGE and call(arena(n_rewards=-1)) == _lib.E_RANGE
        assert call(arena(n=-1)) == _lib.E_RANGE
        for bad in (-1, 2, 7):
            assert call(arena(robot=bad)) == _lib.E_ARG, bad
        for bad in (-1, 2, 8, 32, 63, 128):
            assert call(arena(lanes=bad)) == _lib.E_ARG, bad
        # nothing to do: no launch, so no error either
        assert call(arena(n=0)) == _lib.OK
        assert call(arena(n=0, n_rewards=0, rewards=None, lanes=16, robot=cc.WHEEL)) == _lib.OK
    for name in ('action', 'reward', 'done', 'wall'):
        assert step(arena(), **{name: None}) == _lib.E_ARG, name
    assert step(arena(), reward=p + 4) == _lib.E_ARG
    assert reset(arena(), fallbacks=None) == _lib.E_ARG and reset(arena(), fallbacks=p + 2) == _lib.E_ARG
    with pytest.raises(IndexError, match='1025 edges'):
        _lib.check(step(arena(n_edges=1025)))
    with pytest.raises(AssertionError, match='8 lanes per instance'):
        _lib.check(reset(arena(lanes=8)))
    with pytest.raises(IndexError, match='33 reward rows'):
        _lib.check(step(arena(n_rewards=33)))
    with pytest.raises(AssertionError, match='robot type 2'):
        _lib.check(step(arena(robot=2)))
