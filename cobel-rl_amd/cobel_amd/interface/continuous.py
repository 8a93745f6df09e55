"""Vectorised continuous 2D arena on the HIP library — ``cobel.interface.Continuous2D``
(interface/continuous.py:21-438).

``Continuous2D(robot_type, room, spawn, obstacles, rewards, simulator=None, widget=None, rng=None)``
as in the reference, plus ``n_envs``, ``seed``, ``device`` and ``instance_base`` as ``Gridworld`` and
``Topology`` have them.  ``room``, ``spawn`` and every obstacle may be a
``continuous_tools.Polygon``, a ``[V, 2]`` array-like or any object with ``.exterior.coords`` and
``.interiors`` — a shapely polygon works, shapely itself is never imported.

The arena is compiled once (``build_geometry``) into a table of directed edges with the interior
to their left; ``step`` and ``reset`` are ``cobel_c2d_step`` / ``cobel_c2d_reset`` over all
instances.  The rule that replaces shapely's clipping (the robot stops ``|buffer|`` inside the
wall it runs into) is written out in ``include/cobel_hip.h`` and INTEGRATION.md.

The scalar attributes (``step_size``, ``body_radius``, ``wheel_distance``, ``buffer``,
``punish_wall``) are read at every call; an edit of ``R`` reaches the device with the next
``sync_world()``, which ``step``, ``reset`` and the agents call.  The geometry is fixed.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..misc.continuous_tools import Polygon
from ..spaces import Box, Discrete
from .gridworld import _as_seed
from .interface import Interface

GRID = 64            # the constructor's acceptance estimate: GRID x GRID cell centres
MIN_ACCEPTED = 256   # ... of which at least 1 / 16 must be accepted


# -- geometry on the host ---------------------------------------------------------------------------
def rings_of(shape) -> list:
    """``[exterior, hole, ...]`` as open ``[V, 2]`` float64 vertex arrays."""
    if hasattr(shape, 'exterior'):
        rings = [np.array(shape.exterior.coords, dtype=np.float64)]
        rings += [np.array(r.coords, dtype=np.float64) for r in shape.interiors]
    else:
        rings = [np.array(shape, dtype=np.float64)]
    out = []
    for r in rings:
        r = r.reshape(len(r), -1)[:, :2]
        if len(r) > 1 and np.array_equal(r[0], r[-1]):
            r = r[:-1]
        if len(r) < 3:
            raise ValueError('a ring needs at least three vertices')
        out.append(np.ascontiguousarray(r))
    return out


def signed_area(ring: np.ndarray) -> float:
    x, y = ring[:, 0], ring[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def oriented(ring: np.ndarray, ccw: bool) -> np.ndarray:
    return ring if (signed_area(ring) > 0) == ccw else ring[::-1].copy()


def edge_table(rings: list) -> np.ndarray:
    """``[8, E]``: ax, ay, bx, by, ex, ey, nx, ny of every edge of ``rings`` (the first ring the
    exterior, the others holes), zero-length edges dropped."""
    a, b = [], []
    for k, ring in enumerate(rings):
        r = oriented(ring, k == 0)
        a.append(r)
        b.append(np.roll(r, -1, axis=0))
    a, b = np.concatenate(a), np.concatenate(b)
    keep = (a != b).any(axis=1)
    a, b = a[keep], b[keep]
    ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    L = np.sqrt(ex * ex + ey * ey)     # noqa: N806
    return np.ascontiguousarray(np.stack([a[:, 0], a[:, 1], b[:, 0], b[:, 1], ex, ey, -ey / L, ex / L]))


def inside(table: np.ndarray, P: np.ndarray) -> np.ndarray:   # noqa: N803
    """Even-odd rule for points ``[M, 2]`` (the kernel's arithmetic, all points at once)."""
    ax, ay, _, by, ex = (table[k][None, :] for k in range(5))
    px, py = P[:, 0][:, None], P[:, 1][:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        xi = ax + (py - ay) / (by - ay) * ex
    return (((ay > py) != (by > py)) & (px < xi)).sum(axis=1) % 2 == 1


def clear(table: np.ndarray, P: np.ndarray, m: float) -> np.ndarray:   # noqa: N803
    """``inside`` and at least ``m / 2`` away from every edge."""
    ax, ay, _, _, ex, ey = (table[k][None, :] for k in range(6))
    px, py = P[:, 0][:, None], P[:, 1][:, None]
    s = np.clip(((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    qx, qy = ax + s * ex, ay + s * ey
    d2 = (px - qx) * (px - qx) + (py - qy) * (py - qy)
    half = m / 2.0
    return inside(table, P) & (d2 >= half * half).all(axis=1)


def _segments_meet(a: np.ndarray, b: np.ndarray, c: np.ndarray, d: np.ndarray) -> bool:
    """Does any segment a[i]b[i] meet (cross or touch) any segment c[j]d[j]?"""
    def orient(p, q, r):
        return np.sign((q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1])
                       - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0]))

    def on(p, q, r):    # r collinear with pq: within its box?
        return ((np.minimum(p[..., 0], q[..., 0]) <= r[..., 0]) & (r[..., 0] <= np.maximum(p[..., 0], q[..., 0]))
                & (np.minimum(p[..., 1], q[..., 1]) <= r[..., 1]) & (r[..., 1] <= np.maximum(p[..., 1], q[..., 1])))
    A, B, Cc, D = a[:, None, :], b[:, None, :], c[None, :, :], d[None, :, :]   # noqa: N806
    o1, o2, o3, o4 = orient(A, B, Cc), orient(A, B, D), orient(Cc, D, A), orient(Cc, D, B)
    meet = (o1 != o2) & (o3 != o4)
    meet |= (o1 == 0) & on(A, B, Cc)
    meet |= (o2 == 0) & on(A, B, D)
    meet |= (o3 == 0) & on(Cc, D, A)
    meet |= (o4 == 0) & on(Cc, D, B)
    return bool(meet.any())


def _ring_table(ring: np.ndarray) -> np.ndarray:
    return edge_table([ring])


def build_geometry(room, spawn, obstacles, buffer: float = 1e-6) -> dict:
    """The host tables of an arena: ``edges`` ``[8, E]`` (room exterior, the room's own holes, one
    hole per obstacle), ``spawn_edges``, ``box`` (lo_x, lo_y, hi_x, hi_y), ``fallback``, ``limits``
    and ``accepted`` (cell centres of the acceptance grid that a reset would take)."""
    out_of_scope = 'general polygon clipping is out of scope'
    room_rings = rings_of(room)
    holes = list(room_rings[1:])
    for k, obstacle in enumerate(obstacles or []):
        rings = rings_of(obstacle)
        if len(rings) > 1:
            raise ValueError('obstacle %d has holes of its own: %s' % (k, out_of_scope))
        ring = rings[0]
        others = [room_rings[0]] + holes
        a, b = ring, np.roll(ring, -1, axis=0)
        for other in others:
            if _segments_meet(a, b, other, np.roll(other, -1, axis=0)):
                raise ValueError('obstacle %d touches or crosses the border or another obstacle: '
                                 'an obstacle lies strictly inside the room and apart from the '
                                 'others — %s' % (k, out_of_scope))
        if not inside(_ring_table(room_rings[0]), ring[:1])[0]:
            raise ValueError('obstacle %d lies outside the room: %s' % (k, out_of_scope))
        for other in holes:
            if inside(_ring_table(other), ring[:1])[0] or inside(_ring_table(ring), other[:1])[0]:
                raise ValueError('obstacle %d overlaps another hole of the room: %s'
                                 % (k, out_of_scope))
        holes.append(ring)
    env_rings = [room_rings[0]] + holes
    edges = edge_table(env_rings)
    if edges.shape[1] > _lib.C2D_MAX_EDGES:
        raise ValueError('the arena has %d edges: Continuous2D serves up to %d'
                         % (edges.shape[1], _lib.C2D_MAX_EDGES))
    ext = env_rings[0]
    limits = np.array([ext[:, 0].min(), ext[:, 1].min(), ext[:, 0].max(), ext[:, 1].max()])
    m = abs(float(buffer))
    spawn_edges, box = edges, limits.copy()
    if spawn is not None:
        s_rings = rings_of(spawn)
        s_table = edge_table(s_rings)
        s_vertices, e_vertices = np.concatenate(s_rings), np.concatenate(env_rings)
        overlaps = inside(edges, s_vertices).any() or inside(s_table, e_vertices).any() or \
            _segments_meet(s_table[0:2].T, s_table[2:4].T, edges[0:2].T, edges[2:4].T)
        if overlaps:      # continuous.py:153-156
            if s_table.shape[1] > _lib.C2D_MAX_EDGES:
                raise ValueError('the spawn area has %d edges: Continuous2D serves up to %d'
                                 % (s_table.shape[1], _lib.C2D_MAX_EDGES))
            spawn_edges = s_table
            s_ext = s_rings[0]
            box = np.array([max(s_ext[:, 0].min(), limits[0]), max(s_ext[:, 1].min(), limits[1]),
                            min(s_ext[:, 0].max(), limits[2]), min(s_ext[:, 1].max(), limits[3])])
    centre = (np.arange(GRID) + 0.5) / GRID
    gx = box[0] + (box[2] - box[0]) * centre
    gy = box[1] + (box[3] - box[1]) * centre
    P = np.stack([np.tile(gx, GRID), np.repeat(gy, GRID)], axis=1)    # noqa: N806  (row by row)
    ok = inside(spawn_edges, P) & clear(edges, P, m)
    accepted = int(ok.sum())
    if accepted < MIN_ACCEPTED:
        raise ValueError('spawn area too thin for rejection sampling: %d of %d grid points of its '
                         'bounding box are valid starts (at least %d are needed)'
                         % (accepted, GRID * GRID, MIN_ACCEPTED))
    return dict(edges=edges, spawn_edges=np.ascontiguousarray(spawn_edges), box=box,
                fallback=P[int(np.argmax(ok))].copy(), limits=limits, accepted=accepted)


def reward_rows(rewards) -> np.ndarray:
    """``R`` as ``[K, 3]`` float64 (the templates return an empty array for "no goal")."""
    r = np.asarray(rewards, dtype=np.float64)
    if r.size == 0:
        return np.zeros((0, 3))
    r = r.reshape(-1, 3)
    if len(r) > _lib.C2D_MAX_REWARDS:
        raise ValueError('%d reward rows: Continuous2D serves up to %d' % (len(r), _lib.C2D_MAX_REWARDS))
    return np.ascontiguousarray(r)


class Continuous2D(Interface):
    def __init__(self, robot_type: str, room, spawn, obstacles, rewards, simulator=None,
                 widget=None, rng=None, n_envs: int = 1, seed: int | None = None, device=None,
                 instance_base: int = 0) -> None:
        super().__init__(widget)
        assert robot_type in ('step', 'wheel'), "robot_type is 'step' or 'wheel'"
        assert simulator is None, 'Continuous2D takes no simulator (the reference ignores it)'
        self.rng = rng
        self.R = rewards
        self.room = room
        self.obstacles = [] if obstacles is None else obstacles
        self.buffer = -(10 ** -6)
        self.geometry = build_geometry(room, spawn, self.obstacles, self.buffer)
        self.limits = self.geometry['limits']
        self.spawn = spawn if self.geometry['spawn_edges'] is not self.geometry['edges'] else room
        self.punish_wall = False
        self.type = robot_type
        self.simulator = None
        wheel = robot_type == 'wheel'
        self.observation_space = Box(low=0.0, high=1.0, shape=(3 if wheel else 2,))
        self.action_space = Discrete(3 if wheel else 4)
        self.body_radius = 0.05
        self.wheel_radius = 0.02
        self.wheel_distance = 0.1
        self.step_size = 0.015
        self.n_envs = int(n_envs)
        self.seed = _as_seed(rng) if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.instance_base = int(instance_base)
        self.lanes_per_instance = 0     # 0: the library's planner; 1, 4, 16, 64 (same results)
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        N, dev = self.n_envs, self.device    # noqa: N806
        self._edges = torch.as_tensor(self.geometry['edges'], device=dev).contiguous()
        self._spawn_edges = torch.as_tensor(self.geometry['spawn_edges'], device=dev).contiguous()
        self._R_host = reward_rows(self.R).copy()
        self._R_dev = torch.zeros((_lib.C2D_MAX_REWARDS, 3), dtype=torch.float64, device=dev)
        self._R_dev[:len(self._R_host)] = torch.as_tensor(self._R_host)
        self.state = torch.zeros((N, 3), dtype=torch.float64, device=dev)
        self.env_ctr = torch.zeros(N, dtype=torch.int32, device=dev)
        self._reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self._done = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._wall = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._fallbacks = torch.zeros(1, dtype=torch.int32, device=dev)
        self.observation = None
        self.current_step = 0
        self.initialize_visualization()
        if self.device.type == 'cuda':
            self.reset()      # continuous.py:183

    # -- the arena as the library takes it --------------------------------------------------------
    def descriptor(self) -> '_lib.C2D':
        """``cobel_c2d_t`` with the scalar attributes as they are now."""
        c, g = _lib.C2D(), self.geometry
        c.edges, c.spawn_edges = _lib.ptr(self._edges), _lib.ptr(self._spawn_edges)
        c.rewards = _lib.ptr(self._R_dev)
        c.state, c.env_ctr = _lib.ptr(self.state), _lib.ptr(self.env_ctr)
        c.box = (C.c_double * 4)(*g['box'])
        c.fallback = (C.c_double * 2)(*g['fallback'])
        c.step_size, c.body_radius = float(self.step_size), float(self.body_radius)
        c.wheel_distance, c.buffer = float(self.wheel_distance), float(self.buffer)
        c.seed = self.seed
        c.n, c.n_edges, c.n_spawn_edges = self.n_envs, self._edges.shape[1], self._spawn_edges.shape[1]
        c.n_rewards = len(self._R_host)
        c.robot_type = _lib.C2D_WHEEL if self.type == 'wheel' else _lib.C2D_STEP
        c.punish_wall = int(bool(self.punish_wall))
        c.lanes_per_instance = int(self.lanes_per_instance)
        c.instance_base = self.instance_base
        return c

    def sync_world(self) -> bool:
        """Compare ``R`` with what the device holds and push it, in stream order, if it differs.
        Returns whether anything was pushed."""
        rows = reward_rows(self.R)
        if rows.shape == self._R_host.shape and np.array_equal(rows, self._R_host):
            return False
        self._R_host = rows.copy()
        if len(rows):
            self._R_dev[:len(rows)].copy_(torch.as_tensor(rows), non_blocking=False)
        return True

    def _on_device(self) -> None:
        if self.device.type != 'cuda':
            raise _lib.CobelHipError('this Continuous2D was built on the host (device=%s): step and '
                                     'reset need a GPU' % self.device)

    def _stream(self):
        return _lib.current_stream(self.device)

    # -- reference surface ------------------------------------------------------------------------
    def observe(self) -> torch.Tensor:
        """``[N, 2]`` (step robot) or ``[N, 3]`` float64 on the device, a copy."""
        return self.state.clone() if self.type == 'wheel' else self.state[:, :2].contiguous()

    def _observation(self):
        obs = self.observe()
        self.observation = obs[0].cpu().numpy() if self.n_envs == 1 else obs
        return self.observation.copy() if self.n_envs == 1 else obs

    def step(self, action):
        self._on_device()
        N = self.n_envs    # noqa: N806
        if N == 1 and not torch.is_tensor(action):
            a = int(action)
            assert 0 <= a < int(self.action_space.n), 'Invalid action type!'
            act = torch.full((1,), a, dtype=torch.uint8, device=self.device)
        else:
            act = torch.as_tensor(action, device=self.device).to(torch.uint8).contiguous()
            assert act.shape == (N,), 'one action per instance'
        self.sync_world()
        c = self.descriptor()
        _lib.check(_lib.lib().cobel_c2d_step(C.byref(c), _lib.ptr(act), _lib.ptr(self._reward),
                                             _lib.ptr(self._done), _lib.ptr(self._wall),
                                             self._stream()))
        self.update_visualization()
        self.current_step += 1
        obs = self._observation()
        if N == 1:
            end = bool(self._done[0].item())
            return obs, float(self._reward[0].item()), end, end, {}
        done = self._done.bool()
        return obs, self._reward, done, done, {}

    def reset(self, mask=None):
        self._on_device()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            assert m.shape == (self.n_envs,), 'one mask entry per instance'
        self.sync_world()
        c = self.descriptor()
        _lib.check(_lib.lib().cobel_c2d_reset(C.byref(c), _lib.ptr(m), _lib.ptr(self._fallbacks),
                                              self._stream()))
        if mask is None:
            self.current_step = 0
        return self._observation(), {}

    @property
    def reset_fallbacks(self) -> int:
        """Resets that found no start among 1 024 candidates and took the fallback point."""
        return int(self._fallbacks.item())

    @property
    def wall_hit(self):
        """Whether the last step ran into a wall: a bool, or ``[N]`` on the device."""
        return bool(self._wall[0].item()) if self.n_envs == 1 else self._wall.bool()

    def get_position(self):
        pos = self.state[:, :2].cpu().numpy()
        return pos[0].copy() if self.n_envs == 1 else pos

    def initialize_visualization(self) -> None:
        pass

    def update_visualization(self) -> None:
        pass


__all__ = ['Continuous2D', 'Polygon', 'build_geometry']
