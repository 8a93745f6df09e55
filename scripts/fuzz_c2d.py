#!/usr/bin/env python3
"""Randomised parity sweep for the continuous 2D arena (csrc/continuous.hip) against the float64
restatement of tests/c2d_common.py.

    python scripts/fuzz_c2d.py [first_seed] [count]

Seeds below 10^6 are step-robot cases: a star-shaped exterior of 3 .. 40 vertices (one seed in 16
is forced to 3 edges, one to 1 024), an axis-aligned rectangle or the eight maze (horizontal edges:
``by - ay == 0`` in the ray test), 0 .. 4 polygonal holes, a spawn table that differs from the arena
in half the cases, 0 .. 4 reward rows (some overlapping), random step size, wall punishment, instance
count, instance base and two lane mappings.  Starts are planted near walls; a few have the y of a
vertex to the bit and move horizontally (the ray of the inside test passes through the vertex), a
few stand exactly one step from an axis-aligned wall (the target lies on the wall, t == 1).
Counters start near 0xFFFFFFFF, a masked reset happens mid-walk.  State, reward, done, wall and
counters after every step are compared with np.array_equal, and the sentinel frames around the
outputs stay untouched.

Seeds from 10^6 on are wheel-robot cases, stepped one step at a time from the restatement's own
state: flags, rewards and theta bit for bit, positions within 1e-13 (the bound derived in
tests/test_gpu_c2d.py for arenas inside the unit box and step sizes up to 0.03).  An instance-step is
left out only where the restatement's own diagnostics show a discrete decision within 1e-9 of its
threshold or a hit at an incidence below 0.1 rad; ``WHEEL_STATS`` counts them.
"""
from __future__ import annotations

import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'cobel-rl_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

WHEEL_SEEDS = 1_000_000
LANES = (0, 1, 4, 16, 64)
COUNTS = (1, 5, 63, 64, 65, 257)
POSITION_BOUND, MARGIN, INCIDENCE = 1e-13, 1e-9, 0.1
# per wheel case run: (seed, instance-steps, left out, largest position difference)
WHEEL_STATS: list = []


# -- geometry ---------------------------------------------------------------------------------------
def _star(r, k):
    # sorted random angles, one per sector of 2 pi / k (so that no gap reaches pi: the centre
    # stays inside, and no two vertices of a 1 024-gon coincide)
    jitter = 0.8 if k >= 4 else 0.4
    ang = r.uniform(0.0, 2.0 * math.pi) + 2.0 * math.pi * (np.arange(k) + r.uniform(0.0, jitter, k)) / k
    rad = r.uniform(0.25, 0.5, k)
    return [(0.5 + float(q) * math.cos(float(a)), 0.5 + float(q) * math.sin(float(a)))
            for a, q in zip(ang, rad)]


def _rings(r, forced=None):
    """-> (kind, exterior, holes)."""
    import c2d_common as cc
    if forced is not None:
        return 'star', _star(r, forced), []
    u = r.random()
    if u < 0.2:
        return 'eight', *cc.eight_maze_rings(float(r.uniform(0.3, 0.5)), float(r.uniform(0.2, 0.3)),
                                             float(r.uniform(0.08, 0.12)))
    if u < 0.4:
        x0, y0 = float(r.uniform(0.0, 0.3)), float(r.uniform(0.0, 0.3))
        x1, y1 = float(r.uniform(0.6, 1.0)), float(r.uniform(0.6, 1.0))
        ext = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        kind = 'rectangle'
    else:
        ext, kind = _star(r, int(r.integers(3, 41))), 'star'
    holes = []
    for _ in range(int(r.integers(0, 5))):
        for _ in range(20):
            T = cc.table(ext, holes)
            cx, cy = float(r.uniform(0.1, 0.9)), float(r.uniform(0.1, 0.9))
            hole = cc.gon(cx, cy, float(r.uniform(0.02, 0.05)), int(r.integers(3, 7)),
                          float(r.uniform(0.0, 2.0 * math.pi)))
            H = cc.table(hole)
            mine = hole + [((a[0] + b[0]) / 2, (a[1] + b[1]) / 2) for a, b in zip(hole, hole[1:] + hole[:1])]
            # no closer than 0.05 to another ring: its vertices and edge midpoints to every edge so
            # far, every vertex so far to its edges
            if not cc.inside(T, cx, cy):
                continue
            if any(cc.edge_distance2(T, x, y).min() < 0.05 ** 2 for x, y in mine):
                continue
            if any(cc.edge_distance2(H, float(x), float(y)).min() < 0.05 ** 2
                   for x, y in zip(T[cc.AX], T[cc.AY])):
                continue
            holes.append(hole)
            break
    return kind, ext, holes


def _first_grid_point(T, S, box):
    """``c2d_common.first_grid_point`` without the count: it stops at the first accepted centre."""
    import c2d_common as cc
    for iy in range(64):
        for ix in range(64):
            x = box[0] + (box[2] - box[0]) * ((ix + 0.5) / 64)
            y = box[1] + (box[3] - box[1]) * ((iy + 0.5) / 64)
            if cc.inside(S, x, y) and cc.clear(T, x, y):
                return (x, y)
    return None


def _arena(r, forced=None):
    import c2d_common as cc
    kind, ext, holes = _rings(r, forced)
    T = cc.table(ext, holes)
    S, box = T, cc.bounds(T)
    if forced is None and r.random() < 0.5:
        for _ in range(20):
            cx, cy = float(r.uniform(0.3, 0.7)), float(r.uniform(0.3, 0.7))
            rad = float(r.uniform(0.08, 0.25))
            S2 = cc.table(cc.gon(cx, cy, rad, int(r.integers(3, 9)), float(r.uniform(0.0, 6.0))))
            box2 = cc.bounds(S2) if r.random() < 0.5 else box
            if _first_grid_point(T, S2, box2) is not None:
                S, box = S2, box2
                break
    fallback = _first_grid_point(T, S, box)
    assert fallback is not None
    rows = []
    for _ in range(int(r.integers(0, 5))):
        if rows and r.random() < 0.4:       # in reach of an earlier row as well: the first wins
            x, y = rows[-1][0] + float(r.uniform(-0.05, 0.05)), rows[-1][1] + float(r.uniform(-0.05, 0.05))
        else:
            while True:
                x, y = float(r.uniform(0.05, 0.95)), float(r.uniform(0.05, 0.95))
                if cc.inside(T, x, y):
                    break
        rows.append([x, y, float(r.choice([10.0, 5.0, 1.0, -2.0, 0.5]))])
    R = np.array(rows, dtype=np.float64).reshape(-1, 3)
    return kind, T, S, box, fallback, R


def _two_lanes(r):
    return tuple(int(x) for x in r.choice(LANES, 2, replace=False))


# -- cases ------------------------------------------------------------------------------------------
def draw_case(seed: int) -> dict:
    return _draw_wheel(seed) if seed >= WHEEL_SEEDS else _draw_step(seed)


def _draw_step(seed: int) -> dict:
    import c2d_common as cc
    r = np.random.default_rng(seed)
    forced = {3: 3, 11: 1024}.get(seed % 16)
    kind, T, S, box, fallback, R = _arena(r, forced)
    E = T.shape[1]
    n = int(r.choice(COUNTS))
    step_size = float(r.uniform(0.005, 0.03))
    steps = int(r.integers(12, 41))
    steps = max(6, min(steps, 4000 // n, 4_000_000 // (n * (256 + E))))
    params = dict(cc.DEFAULTS, step_size=step_size, punish_wall=int(r.integers(2)))
    start = np.zeros((n, 3))
    start[:, :2] = cc.planted_starts(T, n, r)
    actions = cc.held_actions(n, steps, 4, r)
    planted = {'vertex': [], 'wall': []}
    free = list(r.permutation(n))
    # the y of a vertex to the bit, moving horizontally: every point visited keeps that y
    for _ in range(min(4, len(free))):
        for _ in range(30):
            e = int(r.integers(E))
            vy = float(T[cc.AY][e])
            x = float(T[cc.AX][e]) + float(r.choice([-1.0, 1.0])) * float(r.uniform(0.002, 0.1))
            if cc.clear(T, x, vy):
                i = int(free.pop())
                start[i, :2] = x, vy
                actions[:, i] = int(r.choice([0, 2]))
                planted['vertex'].append(i)
                break
    # exactly one step from an axis-aligned wall: the target lies on the wall
    walls = [e for e in range(E) if T[cc.EX][e] == 0.0 or T[cc.EY][e] == 0.0]
    for _ in range(min(4, len(free)) if walls else 0):
        for _ in range(30):
            e = int(walls[int(r.integers(len(walls)))])
            s = float(r.uniform(0.1, 0.9))
            wx, wy = float(T[cc.AX][e] + s * T[cc.EX][e]), float(T[cc.AY][e] + s * T[cc.EY][e])
            x, y = wx + step_size * float(T[cc.NX][e]), wy + step_size * float(T[cc.NY][e])
            a = [k for k, mv in enumerate(cc.MOVES)
                 if (mv[0], mv[1]) == (-float(T[cc.NX][e]), -float(T[cc.NY][e]))]
            if not a or not cc.clear(T, x, y):
                continue
            tx, ty, _ = cc.target_of(cc.STEP, x, y, 0.0, a[0], params)
            if (tx, ty) != (wx, wy):        # (x0 + s) - s is not always x0
                continue
            i = int(free.pop())
            start[i, :2] = x, y
            actions[0, i] = a[0]
            planted['wall'].append(i)
            break
    ctr0 = (2 * r.integers(0, 50, n)).astype(np.uint32)
    near = r.random(n) < 0.3
    ctr0[near] = (0xFFFFFFFE - 2 * r.integers(0, 6, int(near.sum()))).astype(np.uint32)
    return dict(kind='step', seed=seed, arena=kind, T=T, S=S, box=box, fallback=fallback, R=R, n=n,
                steps=steps, params=params, start=start, actions=actions, planted=planted,
                ctr0=ctr0, reset_at=steps // 2, mask=(r.random(n) < 0.3).astype(np.uint8),
                base=int(r.integers(0, 100_000)), rng_seed=int(r.integers(1, 1 << 31)),
                lanes=_two_lanes(r))


def _draw_wheel(seed: int) -> dict:
    import c2d_common as cc
    r = np.random.default_rng(seed)
    kind, T, S, box, fallback, R = _arena(r)
    E = T.shape[1]
    n, steps = 48, 12
    params = dict(cc.DEFAULTS, step_size=float(r.uniform(0.005, 0.03)), punish_wall=int(r.integers(2)))
    state = np.zeros((n, 3))
    for i in range(n):
        while True:
            e, s, d = int(r.integers(E)), r.uniform(0.1, 0.9), r.uniform(0.004, 0.03)
            x = float(T[cc.AX][e] + s * T[cc.EX][e] + d * T[cc.NX][e])
            y = float(T[cc.AY][e] + s * T[cc.EY][e] + d * T[cc.NY][e])
            if cc.clear(T, x, y):
                break
        heading = math.atan2(-float(T[cc.NY][e]), -float(T[cc.NX][e])) + r.uniform(-1.0, 1.0)
        if i < 6 and len(R):     # just outside the reach of the first reward, heading at it
            away, dist = r.uniform(0.0, cc.TWO_PI), 0.1 + r.uniform(0.003, 0.04)
            qx, qy = float(R[0][0]) + dist * math.cos(away), float(R[0][1]) + dist * math.sin(away)
            if cc.clear(T, qx, qy):
                x, y, heading = qx, qy, away + math.pi + r.uniform(-0.3, 0.3)
        state[i] = x, y, cc.py_mod(heading, cc.TWO_PI)
    actions = np.where(r.random((steps, n)) < 0.8, 2, r.integers(0, 2, (steps, n))).astype(np.uint8)
    actions[r.random((steps, n)) < 0.02] = 3      # not an action of this robot
    return dict(kind='wheel', seed=seed, arena=kind, T=T, S=S, box=box, fallback=fallback, R=R, n=n,
                steps=steps, params=params, start=state, actions=actions, lanes=_two_lanes(r))


def describe(c: dict) -> str:
    return ('seed %(seed)d %(kind)s robot, %(arena)s' % c
            + ' E=%d spawn %s rewards=%d n=%d steps=%d step_size=%.4f punish=%d lanes=%s'
            % (c['T'].shape[1], 'own' if c['S'] is not c['T'] else 'arena', len(c['R']), c['n'],
               c['steps'], c['params']['step_size'], c['params']['punish_wall'], c['lanes'])
            + (' base=%d planted=%s' % (c['base'], {k: len(v) for k, v in c['planted'].items()})
               if c['kind'] == 'step' else ''))


# -- the restatement alone --------------------------------------------------------------------------
def run_reference(c: dict) -> dict:
    """The restatement's record of a case, and counts of what it contains."""
    import c2d_common as cc
    T, R, n, p = c['T'], c['R'], c['n'], c['params']
    seen = dict(wall=0, guard=0, done=0, later_candidate=0, wrapped=0, fell_back=0, steps=0,
                left_out=0)
    if c['kind'] == 'wheel':
        state = c['start'].copy()
        before, after, use = [], [], []
        for t in range(c['steps']):
            before.append(state.copy())
            reward, done, wall = np.zeros(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            ok = np.ones(n, dtype=bool)
            for i in range(n):
                d = {}
                state[i], reward[i], done[i], wall[i] = cc.step(T, R, cc.WHEEL, state[i],
                                                                int(c['actions'][t, i]), p, d)
                if d and (d['margin'] < MARGIN or d.get('phi', math.pi) < INCIDENCE):
                    ok[i] = False
            seen['steps'] += n
            seen['left_out'] += int((~ok).sum())
            seen['wall'] += int(wall.sum())
            seen['done'] += int(done.sum())
            after.append((state.copy(), reward, done, wall))
            use.append(ok)
        return dict(before=before, after=after, use=use, seen=seen)

    def reset_one(i, state, ctr):
        s, new, fell, k = cc.reset(T, c['S'], c['box'], c['fallback'], cc.STEP, c['rng_seed'],
                                   c['base'] + i, int(ctr[i]))
        seen['fell_back'] += int(fell)        # (1 024 candidates refused: a sliver of a spawn area)
        seen['later_candidate'] += int(not fell and k > 0)
        seen['wrapped'] += int(new < int(ctr[i]))
        state[i], ctr[i] = s, new

    state, ctr = np.zeros((n, 3)), c['ctr0'].copy()
    for i in range(n):
        reset_one(i, state, ctr)
    first = (state.copy(), ctr.copy())
    state = c['start'].copy()
    records = []
    for t in range(c['steps']):
        reward, done, wall = np.zeros(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i in range(n):
            old = state[i].copy()
            state[i], reward[i], done[i], wall[i] = cc.step(T, R, cc.STEP, state[i],
                                                            int(c['actions'][t, i]), p)
            seen['guard'] += int(wall[i] and np.array_equal(old, state[i]))
        seen['wall'] += int(wall.sum())
        seen['done'] += int(done.sum())
        seen['steps'] += n
        if t == c['reset_at']:
            for i in np.flatnonzero(c['mask']):
                reset_one(int(i), state, ctr)
        records.append((state.copy(), reward, done, wall, ctr.copy()))
    return dict(first=first, records=records, seen=seen)


# -- the device against it --------------------------------------------------------------------------
def run_case(c: dict) -> list:
    import torch
    import c2d_common as cc
    from test_gpu_c2d import Arena
    ref = run_reference(c)
    bad = []

    def same(got, want, what):
        if got.dtype != want.dtype or not np.array_equal(got, want):
            bad.append('%s at %s' % (what, np.argwhere(got != want)[:3].tolist()))

    def arena(lanes, robot, **kw):
        return Arena(torch, c['T'], c['R'], c['n'], S=c['S'], box=c['box'], fallback=c['fallback'],
                     robot=robot, lanes=lanes, **kw, **c['params'])

    names = ('state', 'reward', 'done', 'wall', 'counters')
    try:
        if c['kind'] == 'step':
            for lanes in c['lanes']:
                A = arena(lanes, cc.STEP, seed=c['rng_seed'], base=c['base'])
                A.ctr.copy_(torch.as_tensor(c['ctr0'].view(np.int32), device='cuda'))
                A.reset()
                state, _, _, _, ctr = A.get()
                same(state, ref['first'][0], 'first reset: state, lanes %d' % lanes)
                same(ctr, ref['first'][1], 'first reset: counters, lanes %d' % lanes)
                A.put(c['start'])
                for t, want in enumerate(ref['records']):
                    A.step(c['actions'][t])
                    if t == c['reset_at']:
                        A.reset(c['mask'])
                    for g, w, what in zip(A.get(), want, names):
                        same(g, w, '%s after step %d, lanes %d' % (what, t, lanes))
                    if bad:
                        return bad
                if int(A.fallbacks.item()) != ref['seen']['fell_back']:
                    bad.append('fallbacks: %d, not %d' % (int(A.fallbacks.item()), ref['seen']['fell_back']))
            return bad
        worst, outs = 0.0, {}
        for lanes in c['lanes']:
            A = arena(lanes, cc.WHEEL)
            outs[lanes] = []
            for t in range(c['steps']):
                A.put(ref['before'][t])
                A.step(c['actions'][t])
                state, reward, done, wall, _ = A.get()
                ws, wr, wd, ww = ref['after'][t]
                use = ref['use'][t]
                same(reward[use], wr[use], 'reward, step %d, lanes %d' % (t, lanes))
                same(done[use], wd[use], 'done, step %d, lanes %d' % (t, lanes))
                same(wall[use], ww[use], 'wall, step %d, lanes %d' % (t, lanes))
                same(state[use, 2], ws[use, 2], 'theta, step %d, lanes %d' % (t, lanes))
                if use.any():
                    worst = max(worst, float(np.abs(state[use, :2] - ws[use, :2]).max()))
                outs[lanes].append(state)
        for t in range(c['steps']):
            same(outs[c['lanes'][1]][t], outs[c['lanes'][0]][t], 'the two mappings differ, step %d' % t)
        WHEEL_STATS.append((c['seed'], ref['seen']['steps'], ref['seen']['left_out'], worst))
        if not worst <= POSITION_BOUND:
            bad.append('largest position difference %.3e above %.0e' % (worst, POSITION_BOUND))
    except AssertionError as err:       # (a sentinel frame was written to)
        bad.append(str(err)[:300])
    return bad


def main() -> int:
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    failed, t0 = [], time.time()
    for seed in range(first, first + count):
        c = draw_case(seed)
        try:
            bad = run_case(c)
        except Exception as e:       # (not a mismatch: nothing more is started on the device)
            print('ERROR %s: %s' % (type(e).__name__, str(e)[:300]), describe(c), flush=True)
            return 2
        if bad:
            failed.append(seed)
            print('MISMATCH', bad[:6], describe(c), flush=True)
        if (seed - first) % 10 == 9:
            print('... %d cases, %d failing, %.0f s' % (seed - first + 1, len(failed), time.time() - t0),
                  flush=True)
    print('cases %d, failing %d: %s' % (count, len(failed), failed))
    if WHEEL_STATS:
        total, out = sum(s[1] for s in WHEEL_STATS), sum(s[2] for s in WHEEL_STATS)
        print('wheel robot: %d of %d instance-steps left out (%.2f %%), largest position difference '
              '%.3e (bound %.0e)' % (out, total, 100.0 * out / total, max(s[3] for s in WHEEL_STATS),
                                     POSITION_BOUND))
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
