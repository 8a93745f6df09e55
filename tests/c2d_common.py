"""TEST INFRASTRUCTURE for the continuous 2D arena: a float64 restatement of its semantics
(include/cobel_hip.h, "The continuous 2D arena"), one instance at a time, in NumPy operations that
round once each and in the order the definition gives; geometry and template builders written from
the formulas, not through the package; fillers for ``cobel_c2d_t``; seeded cases.

The restatement reads the same eight columns per edge the kernel reads and derives nothing else
from the vertices.  Draws come from ``oracle/philox.py``.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import philox  # noqa: E402

M = 1e-6                     # |env.buffer|
TWO_PI = 2.0 * math.pi
STEP, WHEEL = 0, 1
AX, AY, BX, BY, EX, EY, NX, NY = range(8)
MOVES = ((-1.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, -1.0))


# -- geometry, from the formulas ----------------------------------------------------------------------
def area2(ring) -> float:
    r = np.asarray(ring, dtype=np.float64)
    return float(sum(r[k - 1][0] * r[k][1] - r[k][0] * r[k - 1][1] for k in range(len(r))))


def table(exterior, holes=()) -> np.ndarray:
    """``[8, E]`` for one exterior ring (made counter-clockwise) and hole rings (made clockwise)."""
    cols = []
    for k, ring in enumerate([exterior] + list(holes)):
        r = [tuple(map(float, v)) for v in ring]
        if r[0] == r[-1]:
            r = r[:-1]
        if (area2(r) > 0) != (k == 0):
            r = r[::-1]
        for a, b in zip(r, r[1:] + r[:1]):
            if a == b:
                continue
            ex, ey = b[0] - a[0], b[1] - a[1]
            L = math.sqrt(ex * ex + ey * ey)    # noqa: N806
            cols.append((a[0], a[1], b[0], b[1], ex, ey, -ey / L, ex / L))
    return np.ascontiguousarray(np.array(cols, dtype=np.float64).T)


UNIT_SQUARE = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
WEDGE = [(0.0, 0.0), (1.0, -0.0175), (1.0, 0.0175)]


def gon(cx, cy, r, k, phase=0.0):
    return [(cx + r * math.cos(phase + 2.0 * math.pi * i / k), cy + r * math.sin(phase + 2.0 * math.pi * i / k))
            for i in range(k)]


def open_field_rings():
    """The demo's open field: the unit square, a 0.1 x 0.1 square on its corner at the centre, a
    64-gon of radius 0.05 at (0.9, 0.1) and the triangle (0.05, 0.8667) (0.15, 0.8667) (0.1, 0.9667)
    — 4 + 4 + 64 + 3 = 75 edges."""
    d = 0.05 * math.sqrt(2.0)
    diamond = [(0.5, 0.5 - d), (0.5 + d, 0.5), (0.5, 0.5 + d), (0.5 - d, 0.5)]
    h = 0.9 - 0.1 / 3.0
    triangle = [(0.05, h), (0.15, h), (0.1, h + 0.1)]
    return UNIT_SQUARE, [diamond, gon(0.9, 0.1, 0.05, 64), triangle]


def eight_maze_rings(center_height=0.4, lap_width=0.3, cw=0.1):
    height, width = center_height + 2 * cw, 2 * lap_width + 3 * cw
    left = [(cw, cw), (cw + lap_width, cw), (cw + lap_width, height - cw), (cw, height - cw)]
    right = [(x + lap_width + cw, y) for x, y in left]
    return [(0.0, 0.0), (width, 0.0), (width, height), (0.0, height)], [left, right]


def geometries() -> dict:
    """name -> (edge table, rewards).  The reward rows of the open field overlap: both are in reach
    around (0.75, 0.75) and the first must win."""
    of_ext, of_holes = open_field_rings()
    e_ext, e_holes = eight_maze_rings()
    return {
        'square': (table(UNIT_SQUARE), np.zeros((0, 3))),
        'open_field': (table(of_ext, of_holes), np.array([[0.75, 0.75, 10.0], [0.78, 0.75, 5.0]])),
        'eight': (table(e_ext, e_holes), np.array([[0.85, 0.3, 10.0]])),
        'ring1024': (table(gon(0.5, 0.5, 0.5, 1024)), np.array([[0.5, 0.9, 2.0]])),
    }


# -- the restatement -------------------------------------------------------------------------------------
def inside(T, px, py) -> bool:     # noqa: N803
    with np.errstate(divide='ignore', invalid='ignore'):
        xi = T[AX] + (py - T[AY]) / (T[BY] - T[AY]) * T[EX]
    return int(np.count_nonzero(((T[AY] > py) != (T[BY] > py)) & (px < xi))) % 2 == 1


def edge_distance2(T, px, py) -> np.ndarray:    # noqa: N803
    s = ((px - T[AX]) * T[EX] + (py - T[AY]) * T[EY]) / (T[EX] * T[EX] + T[EY] * T[EY])
    s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
    qx, qy = T[AX] + s * T[EX], T[AY] + s * T[EY]
    return (px - qx) * (px - qx) + (py - qy) * (py - qy)


def clear(T, px, py, m=M) -> bool:    # noqa: N803
    half = m / 2.0
    return inside(T, px, py) and bool(np.all(edge_distance2(T, px, py) >= half * half))


def move(T, px, py, tx, ty, m=M, diag=None):    # noqa: N803
    """-> (cx, cy, wall_hit).  ``diag`` (a dict) collects what the wheel tests need: 'phi', the
    incidence angle of a hit, 'guard', whether the guard refused, and 'margin', the least distance
    of any discrete decision from its threshold."""
    dx, dy = tx - px, ty - py
    den = dx * T[NX] + dy * T[NY]
    with np.errstate(divide='ignore', invalid='ignore'):
        sd = (px - T[AX]) * T[NX] + (py - T[AY]) * T[NY]
        t = sd / (-den)
        hx, hy = px + t * dx, py + t * dy
        u = ((hx - T[AX]) * T[EX] + (hy - T[AY]) * T[EY]) / (T[EX] * T[EX] + T[EY] * T[EY])
        valid = (den < 0.0) & (t >= 0.0) & (t <= 1.0) & (u >= -1e-9) & (u <= 1.0 + 1e-9)
    cx, cy, e = tx, ty, -1
    if valid.any():
        e = int(np.argmin(np.where(valid, t, np.inf)))      # (the first of equal minima)
        ts = float(t[e])
        cx = (px + ts * dx) + m * float(T[NX][e])
        cy = (py + ts * dy) + m * float(T[NY][e])
    ok = clear(T, cx, cy, m)
    if diag is not None:
        with np.errstate(divide='ignore', invalid='ignore'):
            # "edge e is hit" = (den < 0) and (0 <= t <= 1) and (u within its bounds): how far a
            # conjunction is from flipping — the least margin of its true terms where all hold,
            # else the largest margin of its false terms (all of them would have to flip).  The
            # sign of den matters only for an edge whose line is within two steps of p.
            in_t, in_u = (t >= 0.0) & (t <= 1.0), (u >= -1e-9) & (u <= 1.0 + 1e-9)
            m_t = np.minimum(np.abs(t), np.abs(t - 1.0))
            m_u = np.minimum(np.abs(u + 1e-9), np.abs(u - (1.0 + 1e-9)))
            both = np.where(in_t & in_u, np.minimum(m_t, m_u),
                            np.where(in_t, m_u, np.where(in_u, m_t, np.maximum(m_t, m_u))))
            margins = [np.where(den < 0.0, both, np.inf),
                       np.where(np.abs(sd) <= 2.0 * math.hypot(dx, dy), np.abs(den), np.inf)]
            if valid.sum() > 1:      # the winner's lead over the runner-up
                margins.append(np.array([np.sort(t[valid])[1] - np.sort(t[valid])[0]]))
            d = np.sqrt(edge_distance2(T, cx, cy))
            margins.append(np.abs(d - m / 2.0))
            straddle_y = np.minimum(np.abs(T[AY] - cy), np.abs(T[BY] - cy))
            xi = T[AX] + (cy - T[AY]) / (T[BY] - T[AY]) * T[EX]
            margins.append(np.where((T[AY] > cy) != (T[BY] > cy), np.abs(cx - xi), np.inf))
            margins.append(np.where(T[AY] != T[BY], straddle_y, np.inf))
        diag['margin'] = min(diag.get('margin', np.inf), min(float(np.min(x)) for x in margins))
        diag['guard'] = not ok
        if e >= 0:
            diag['phi'] = math.asin(min(1.0, float(-den[e]) / math.hypot(dx, dy)))
    if not ok:
        cx, cy = px, py
    return cx, cy, (cx != tx) or (cy != ty)


def py_mod(a: float, b: float) -> float:
    r = math.fmod(a, b)
    if r != 0.0:
        if r < 0.0:
            r += b
    else:
        r = 0.0
    return r


def target_of(robot: int, x, y, th, a: int, p: dict):
    """-> (tx, ty, theta') for an action the robot has."""
    s = p['step_size']
    if robot == STEP:
        return x + MOVES[a][0] * s, y + MOVES[a][1] * s, th
    if a == 2:
        tx, ty, th2 = x + math.cos(th) * s, y + math.sin(th) * s, th
    else:
        v0, v1 = ((0.0, 1.0), (1.0, 0.0))[a]
        v0, v1 = v0 * s, v1 * s
        wd = p['wheel_distance']
        om = (v1 - v0) / wd
        R = 0.5 * wd * ((v0 + v1) / (v1 - v0))    # noqa: N806
        sn = math.sin(th)
        iccx, iccy = x - R * sn, y + R * sn
        relx, rely = x - iccx, y - iccy
        co, so = math.cos(om), math.sin(om)
        tx, ty = (co * relx - so * rely) + iccx, (so * relx + co * rely) + iccy
        th2 = th + th
    return tx, ty, py_mod(th2, TWO_PI)


DEFAULTS = dict(step_size=0.015, body_radius=0.05, wheel_distance=0.1, buffer=-1e-6, punish_wall=0)


def step(T, R, robot: int, state, a: int, p: dict = DEFAULTS, diag=None):    # noqa: N803
    """One step of one instance: -> (new state (x, y, theta), reward, done, wall)."""
    x, y, th = (float(v) for v in state)
    if a >= (4 if robot == STEP else 3):
        return (x, y, th), 0.0, 0, 0
    m = abs(p['buffer'])
    tx, ty, th2 = target_of(robot, x, y, th, a, p)
    cx, cy, hit = move(T, x, y, tx, ty, m, diag)
    reward, done = 0.0, 0
    for row in np.asarray(R, dtype=np.float64).reshape(-1, 3):
        rx, ry = float(row[0]) - cx, float(row[1]) - cy
        dist = math.sqrt(rx * rx + ry * ry)
        if diag is not None:
            diag['margin'] = min(diag['margin'], abs(dist - p['body_radius'] * 2.0))
        if dist <= p['body_radius'] * 2.0:
            reward, done = float(row[2]), 1
            break
    else:
        if hit and p['punish_wall']:
            reward = -10.0
    return (cx, cy, th2), reward, done, int(hit)


def draw(seed: int, g: int, c: int) -> float:
    return float(philox.draw_double(seed, g, c & 0xFFFFFFFF, 0, philox.STREAM_ENV))


def reset(T, S, box, fallback, robot: int, seed: int, g: int, c: int, m=M, refuse_all=False):    # noqa: N803
    """One reset of one instance whose counter is ``c``: -> (state, new counter, fell back, k*)."""
    lox, loy, hix, hiy = (float(v) for v in box)
    for k in range(1024):
        ux, uy = draw(seed, g, c + 2 * k), draw(seed, g, c + 2 * k + 1)
        qx, qy = lox + (hix - lox) * ux, loy + (hiy - loy) * uy
        if not refuse_all and inside(S, qx, qy) and clear(T, qx, qy, m):
            th = TWO_PI * draw(seed, g, c + 2 * k + 2)
            return (qx, qy, 0.0 if robot == STEP else th), (c + 2 * k + 4) & 0xFFFFFFFF, False, k
    th = TWO_PI * draw(seed, g, c + 2048)
    return (float(fallback[0]), float(fallback[1]), 0.0 if robot == STEP else th), \
        (c + 2052) & 0xFFFFFFFF, True, None


def bounds(T) -> np.ndarray:    # noqa: N803
    return np.array([T[AX].min(), T[AY].min(), T[AX].max(), T[AY].max()])


def first_grid_point(T, S, box, m=M):    # noqa: N803
    """The first accepted centre of the 64 x 64 grid over ``box``, row by row, and the count."""
    count, first = 0, None
    for iy in range(64):
        for ix in range(64):
            x = box[0] + (box[2] - box[0]) * ((ix + 0.5) / 64)
            y = box[1] + (box[3] - box[1]) * ((iy + 0.5) / 64)
            if inside(S, x, y) and clear(T, x, y, m):
                count += 1
                if first is None:
                    first = (x, y)
    return first, count


# -- seeded cases ---------------------------------------------------------------------------------------
def planted_starts(T, n: int, rng, lo=1e-5, hi=0.02) -> np.ndarray:    # noqa: N803
    """``[n, 2]`` clear points within ``hi`` of a wall: a point along a random edge, moved inwards."""
    out = np.zeros((n, 2))
    E = T.shape[1]    # noqa: N806
    for i in range(n):
        while True:
            e, s, d = int(rng.integers(E)), rng.uniform(0.05, 0.95), rng.uniform(lo, hi)
            x = float(T[AX][e] + s * T[EX][e] + d * T[NX][e])
            y = float(T[AY][e] + s * T[EY][e] + d * T[NY][e])
            if clear(T, x, y):
                out[i] = x, y
                break
    return out


def held_actions(n: int, steps: int, n_actions: int, rng, stray=0.03) -> np.ndarray:
    """``[steps, n]`` uint8: every instance holds an action for 2 to 8 steps, so that walls are hit;
    a few entries are actions the robot does not have."""
    out = np.zeros((steps, n), dtype=np.uint8)
    for i in range(n):
        t = 0
        while t < steps:
            run = int(rng.integers(2, 9))
            out[t:t + run, i] = rng.integers(n_actions)
            t += run
    wrong = rng.random((steps, n)) < stray
    out[wrong] = rng.choice(np.array([4, 7, 200, 255], dtype=np.uint8), size=int(wrong.sum()))
    return out


class Walk:
    """The restatement's record of one seeded case of the step robot: a reset of every instance,
    planted starts for three in four, ``steps`` steps with a masked reset in the middle."""

    def __init__(self, name: str, n: int, steps: int = 40, seed: int = 0xC2D, punish=1) -> None:
        T, R = geometries()[name]    # noqa: N806
        rng = np.random.default_rng([seed, sum(map(ord, name))])
        self.T, self.R, self.n, self.steps, self.seed = T, R, n, steps, seed
        self.params = dict(DEFAULTS, punish_wall=punish)
        self.box = bounds(T)
        self.fallback, _ = first_grid_point(T, T, self.box)
        self.actions = held_actions(n, steps, 4, rng)
        self.reset_at = steps // 2
        self.mask = (np.arange(n) % 5 == 0).astype(np.uint8)
        ctr = np.zeros(n, dtype=np.uint32)
        state = np.zeros((n, 3))
        for i in range(n):
            state[i], ctr[i], _, _ = reset(T, T, self.box, self.fallback, STEP, seed, i, 0)
        self.after_reset = (state.copy(), ctr.copy())
        planted = planted_starts(T, n, rng)
        keep = np.arange(n) % 4 == 3
        state[~keep, :2] = planted[~keep]
        for i in range(1, n, 16):       # ... and some just outside the reach of the first reward row
            for _ in range(64 if len(R) else 0):
                away, dist = rng.uniform(0.0, TWO_PI), 0.1 + rng.uniform(0.002, 0.03)
                x, y = float(R[0][0]) + dist * math.cos(away), float(R[0][1]) + dist * math.sin(away)
                if clear(T, x, y):
                    state[i, :2] = x, y
                    break
        self.start = state.copy()
        self.records = []     # per step: state, reward, done, wall, ctr (after the step and reset)
        for t in range(steps):
            reward, done, wall = np.zeros(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            for i in range(n):
                state[i], reward[i], done[i], wall[i] = step(T, R, STEP, state[i],
                                                             int(self.actions[t, i]), self.params)
            if t == self.reset_at:
                for i in np.flatnonzero(self.mask):
                    state[i], ctr[i], _, _ = reset(T, T, self.box, self.fallback, STEP, seed, int(i),
                                                   int(ctr[i]))
            self.records.append((state.copy(), reward, done, wall, ctr.copy()))


_WALKS: dict = {}


def walk(name: str, n: int = 300, punish: int = 1) -> Walk:
    """Computed once per geometry for the largest instance count; smaller counts are its first
    rows (an instance depends on its own number, start and actions alone)."""
    key = (name, punish)
    if key not in _WALKS or _WALKS[key].n < n:
        _WALKS[key] = Walk(name, n, punish=punish)
    return _WALKS[key]


class WheelWalk:
    """Seeded case of the wheel robot on the open field: starts near walls, heading roughly at
    them, mostly straight steps.  ``diags[t][i]`` holds the diagnostics of ``move``."""

    def __init__(self, n: int = 48, steps: int = 12, seed: int = 5) -> None:
        T, R = geometries()['open_field']    # noqa: N806
        rng = np.random.default_rng(seed)
        self.T, self.R, self.n, self.steps = T, R, n, steps
        self.params = dict(DEFAULTS, punish_wall=1)
        E = T.shape[1]    # noqa: N806
        state = np.zeros((n, 3))
        for i in range(n):
            while True:
                e, s, d = int(rng.integers(E)), rng.uniform(0.1, 0.9), rng.uniform(0.004, 0.03)
                x = float(T[AX][e] + s * T[EX][e] + d * T[NX][e])
                y = float(T[AY][e] + s * T[EY][e] + d * T[NY][e])
                if clear(T, x, y):
                    break
            heading = math.atan2(-float(T[NY][e]), -float(T[NX][e])) + rng.uniform(-1.0, 1.0)
            if i < 6:       # ... and a few just outside the reach of the first reward, heading at it
                away, dist = rng.uniform(0.0, TWO_PI), 0.1 + rng.uniform(0.003, 0.04)
                x, y = float(R[0][0]) + dist * math.cos(away), float(R[0][1]) + dist * math.sin(away)
                heading = away + math.pi + rng.uniform(-0.3, 0.3)
            state[i] = x, y, py_mod(heading, TWO_PI)
        self.actions = np.where(rng.random((steps, n)) < 0.8, 2, rng.integers(0, 2, (steps, n))) \
            .astype(np.uint8)
        self.actions[rng.random((steps, n)) < 0.02] = 3      # not an action of this robot
        self.before, self.after, self.diags = [], [], []
        for t in range(steps):
            self.before.append(state.copy())
            reward, done, wall = np.zeros(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            diags = []
            for i in range(n):
                d = {}
                state[i], reward[i], done[i], wall[i] = step(T, R, WHEEL, state[i],
                                                             int(self.actions[t, i]), self.params, d)
                diags.append(d)
            self.diags.append(diags)
            self.after.append((state.copy(), reward, done, wall))


_WHEEL: list = []


def wheel_walk() -> WheelWalk:
    if not _WHEEL:
        _WHEEL.append(WheelWalk())
    return _WHEEL[0]


# -- cobel_c2d_t ---------------------------------------------------------------------------------------
def fill(_lib, edges, spawn_edges, rewards, state, env_ctr, n, n_edges, n_spawn, n_rewards, box,
         fallback, robot=STEP, seed=1, base=0, lanes=0, **params):
    """``cobel_c2d_t`` from addresses (ints, or None) and numbers."""
    import ctypes as C    # noqa: N812
    p = dict(DEFAULTS, **params)
    c = _lib.C2D()
    c.edges, c.spawn_edges, c.rewards, c.state, c.env_ctr = edges, spawn_edges, rewards, state, env_ctr
    c.box = (C.c_double * 4)(*[float(v) for v in box])
    c.fallback = (C.c_double * 2)(*[float(v) for v in fallback])
    c.step_size, c.body_radius = p['step_size'], p['body_radius']
    c.wheel_distance, c.buffer = p['wheel_distance'], p['buffer']
    c.seed = seed
    c.n, c.n_edges, c.n_spawn_edges, c.n_rewards = n, n_edges, n_spawn, n_rewards
    c.robot_type, c.punish_wall, c.lanes_per_instance, c.instance_base = robot, p['punish_wall'], lanes, base
    return c


def framed(torch, shape, dtype, fill_value, pad=64):
    """A tensor of ``shape`` inside a larger buffer whose other elements hold ``fill_value``:
    -> (view, check) where ``check()`` asserts that the frame is untouched."""
    count = int(np.prod(shape))
    buf = torch.full((count + 2 * pad,), fill_value, dtype=dtype, device='cuda')
    view = buf[pad:pad + count].view(*shape)

    def check():
        head, tail = buf[:pad].cpu().numpy(), buf[pad + count:].cpu().numpy()
        want = np.full(pad, fill_value, dtype=head.dtype)
        assert np.array_equal(head, want) and np.array_equal(tail, want), 'a kernel wrote outside its output'
    return view, check
