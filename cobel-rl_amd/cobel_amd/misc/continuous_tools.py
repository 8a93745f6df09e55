"""Templates of continuous 2D arenas — ``cobel.misc.continuous_tools`` (misc/continuous_tools.py:13-525)
without shapely: the rooms, spawn areas and obstacles are plain ``Polygon`` values that
``Continuous2D`` compiles into its edge table.

``Polygon`` carries what the interface reads of a shapely polygon: ``.exterior.coords``,
``.interiors`` (rings with ``.coords``) and ``.bounds``.  Rings are closed, the first vertex repeated
at the end, as shapely keeps them.  It offers no boolean operations.

Every template returns the reference's tuple ``(room, spawn, obstacles, rewards)``.
"""
from __future__ import annotations

import numpy as np

__all__ = ['Polygon', 'Ring', 'make_t_maze', 'make_double_t_maze', 'make_two_sided_t_maze',
           'make_eight_maze', 'make_cross_maze', 'make_rectangle', 'make_circle', 'make_triangle']


class Ring:
    """A closed ring of vertices: ``coords`` is ``[V + 1, 2]`` float64, last row == first row."""

    def __init__(self, coords) -> None:
        c = np.array(coords, dtype=np.float64).reshape(-1, 2)
        assert len(c) >= 3, 'a ring needs at least three vertices'
        if not np.array_equal(c[0], c[-1]):
            c = np.concatenate([c, c[:1]])
        self.coords = c

    def __repr__(self) -> str:
        return 'Ring(%d vertices)' % (len(self.coords) - 1)


class Polygon:
    """One exterior ring and any number of interior rings (holes)."""

    def __init__(self, shell, holes=None) -> None:
        self.exterior = Ring(shell)
        self.interiors = [Ring(h) for h in (holes or [])]

    @property
    def bounds(self) -> tuple:
        c = self.exterior.coords
        return (float(c[:, 0].min()), float(c[:, 1].min()), float(c[:, 0].max()), float(c[:, 1].max()))

    def __repr__(self) -> str:
        return 'Polygon(%d vertices, %d holes)' % (len(self.exterior.coords) - 1, len(self.interiors))


ContinuousTemplate = tuple


def _rotate(coords: np.ndarray, degrees: float, origin) -> np.ndarray:
    """Counter-clockwise rotation by ``degrees`` about ``origin`` (shapely.affinity.rotate: cosines
    and sines below 2.5e-16 in magnitude count as zero)."""
    angle = degrees * np.pi / 180.0
    c, s = np.cos(angle), np.sin(angle)
    if abs(c) < 2.5e-16:
        c = 0.0
    if abs(s) < 2.5e-16:
        s = 0.0
    x0, y0 = origin
    x, y = coords[:, 0], coords[:, 1]
    return np.stack([c * x - s * y + (x0 - x0 * c + y0 * s),
                     s * x + c * y + (y0 - x0 * s - y0 * c)], axis=1)


def make_t_maze(stem_length: float, arm_length: float, corridor_width: float,
                goal_arm: str = 'right', reward: float = 1) -> ContinuousTemplate:
    """A T-maze (continuous_tools.py:13-84): the spawn is the foot of the stem, the reward sits at
    the end of the ``goal_arm`` ('left', 'right' or 'none')."""
    assert corridor_width > 0, 'Corridor width must be positive!'
    stem_length = max(corridor_width, stem_length)
    arm_length = max(corridor_width, arm_length)
    height, width = stem_length + corridor_width, arm_length * 2 + corridor_width
    borders = np.array([
        [0, height], [width, height], [width, height - corridor_width],
        [width - arm_length, height - corridor_width], [width - arm_length, 0], [arm_length, 0],
        [arm_length, height - corridor_width], [0, height - corridor_width], [0, height]])
    rewards = np.array([])
    if goal_arm in ['left', 'right']:
        offset = (goal_arm == 'right') * arm_length * 2
        rewards = np.array([[corridor_width / 2 + offset, height - corridor_width / 2, reward]])
    spawn = np.array([
        [arm_length, 0], [arm_length + corridor_width, 0],
        [arm_length + corridor_width, corridor_width], [arm_length, corridor_width],
        [arm_length, 0]])
    return Polygon(borders), Polygon(spawn), [], rewards


def make_double_t_maze(stem_length: float, arm_length: float, corridor_width: float,
                       goal_arm: str = 'right-right', reward: float = 1) -> ContinuousTemplate:
    """A double T-maze (continuous_tools.py:87-178); ``goal_arm`` is 'left-left', 'left-right',
    'right-left', 'right-right' or 'none'."""
    assert corridor_width > 0, 'Corridor width must be positive!'
    stem_length = max(corridor_width, stem_length)
    arm_length = max(corridor_width * 2, arm_length)
    height, width = 2 * stem_length + corridor_width, arm_length * 4 - corridor_width
    cw = corridor_width
    borders = np.array([
        [0, height], [2 * arm_length - cw, height], [2 * arm_length - cw, height - cw],
        [arm_length, height - cw], [arm_length, height - stem_length],
        [3 * arm_length - cw, height - stem_length], [3 * arm_length - cw, height - cw],
        [2 * arm_length, height - cw], [2 * arm_length, height], [width, height],
        [width, height - cw], [width - arm_length + cw, height - cw],
        [width - arm_length + cw, height - stem_length - cw],
        [2 * arm_length, height - stem_length - cw], [2 * arm_length, 0],
        [2 * arm_length - cw, 0], [2 * arm_length - cw, height - stem_length - cw],
        [arm_length - cw, height - stem_length - cw], [arm_length - cw, height - cw],
        [0, height - cw], [0, height]])
    rewards = np.array([])
    if goal_arm in ['left-left', 'left-right', 'right-left', 'right-right']:
        first, second = goal_arm.split('-')
        offset = (first == 'right') * 2 * arm_length + (second == 'right') * 2 * (arm_length - cw)
        rewards = np.array([[cw / 2 + offset, height - cw / 2, reward]])
    spawn = np.array([
        [2 * arm_length - cw, 0], [2 * arm_length, 0], [2 * arm_length, cw],
        [2 * arm_length - cw, cw], [2 * arm_length - cw, 0]])
    return Polygon(borders), Polygon(spawn), [], rewards


def make_two_sided_t_maze(stem_length: float, arm_length: float, corridor_width: float,
                          goal_arm: str = 'right-right', reward: float = 1) -> ContinuousTemplate:
    """A two-sided T-maze, an H on its side (continuous_tools.py:181-265); the spawn is the middle
    of the stem."""
    assert corridor_width > 0, 'Corridor width must be positive!'
    stem_length = max(corridor_width, stem_length)
    arm_length = max(corridor_width, arm_length)
    cw = corridor_width
    height, width = 2 * arm_length + cw, 2 * cw + stem_length
    borders = np.array([
        [0, height], [cw, height], [cw, height - arm_length], [width - cw, height - arm_length],
        [width - cw, height], [width, height], [width, 0], [width - cw, 0],
        [width - cw, arm_length], [cw, arm_length], [cw, 0], [0, 0], [0, height]])
    rewards = np.array([])
    if goal_arm in ['left-left', 'left-right', 'right-left', 'right-right']:
        first, second = goal_arm.split('-')
        offset = np.array([(first == 'right') * (width - cw),
                           (goal_arm in ['left-right', 'right-left']) * (height - cw)])
        rewards = np.array([[cw / 2 + offset[0], cw / 2 + offset[1], reward]])
    s_x, s_y = (width - cw) / 2, arm_length
    spawn = np.array([[s_x, s_y], [s_x + cw, s_y], [s_x + cw, s_y + cw], [s_x, s_y + cw],
                      [s_x, s_y]])
    return Polygon(borders), Polygon(spawn), [], rewards


def make_eight_maze(center_height: float, lap_width: float, corridor_width: float,
                    goal_arm: str = 'right', reward: float = 1) -> ContinuousTemplate:
    """An 8-maze (continuous_tools.py:268-351): a rectangle whose room already has two holes, the
    laps; the spawn is the middle of the centre corridor."""
    assert corridor_width > 0, 'Corridor width must be positive!'
    center_height = max(corridor_width, center_height)
    lap_width = max(corridor_width, lap_width)
    cw = corridor_width
    height = center_height + 2 * cw
    width = lap_width * 2 + 3 * cw
    borders = np.array([[0, 0], [width, 0], [width, height], [0, height], [0, 0]])
    left_lap = np.array([[cw, cw], [cw + lap_width, cw], [cw + lap_width, height - cw],
                         [cw, height - cw], [cw, cw]])
    right_lap = left_lap + np.array([lap_width + cw, 0])
    rewards = np.array([])
    if goal_arm in ['left', 'right']:
        rewards = np.array([[cw / 2 + (goal_arm == 'right') * (width - cw), height / 2, reward]])
    s_x, s_y = lap_width + cw, (height - cw) / 2
    spawn = np.array([[s_x, s_y], [s_x + cw, s_y], [s_x + cw, s_y + cw], [s_x, s_y + cw],
                      [s_x, s_y]])
    return Polygon(borders, [left_lap, right_lap]), Polygon(spawn), [], rewards


def make_cross_maze(arm_length: float, corridor_width: float, goal_arm: str = 'top',
                    reward: float = 1, rotation: float = 0.0) -> ContinuousTemplate:
    """A cross centred at the origin, rotated by ``rotation`` degrees (continuous_tools.py:354-435);
    the spawn is the centre square."""
    assert arm_length > 0, 'The arm length must be positive!'
    assert corridor_width > 0, 'Corridor width must be positive!'
    assert goal_arm in ('left', 'top', 'right', 'bottom'), 'Invalid goal arm!'
    w = corridor_width / 2
    l = w + arm_length  # noqa: E741
    theta = np.deg2rad(rotation)
    R = np.array([(np.cos(theta), -np.sin(theta)), (np.sin(theta), np.cos(theta))])  # noqa: N806
    borders = np.array([(-l, w), (-w, w), (-w, l), (w, l), (w, w), (l, w), (l, -w), (w, -w),
                        (w, -l), (-w, -l), (-w, -w), (-l, -w), (-l, w)])
    for i in range(borders.shape[0]):
        borders[i] = R @ borders[i]
    rewards = np.array([{'left': (-arm_length, 0), 'top': (0, arm_length),
                         'right': (arm_length, 0), 'bottom': (0, -arm_length)}[goal_arm]],
                       dtype=np.float64)
    rewards[0] = R @ rewards[0]
    rewards = np.hstack((rewards, np.full((1, 1), reward)))
    spawn = np.array([(-w, w), (w, w), (w, -w), (-w, -w), (-w, w)])
    for i in range(spawn.shape[0]):
        spawn[i] = R @ spawn[i]
    return Polygon(borders), Polygon(spawn), [], rewards


def make_rectangle(location, width: float, height: float, orientation: float = 0.0) -> Polygon:
    """A rectangular obstacle (continuous_tools.py:438-465): rotated by ``orientation`` degrees
    about its own centre, then moved to ``location``."""
    h, w = height / 2, width / 2
    c = _rotate(np.array([[-w, -h], [w, -h], [w, h], [-w, h], [-w, -h]], dtype=np.float64),
                orientation, (0.0, 0.0))
    return Polygon(c + np.array([location[0], location[1]], dtype=np.float64))


def make_circle(location, radius: float) -> Polygon:
    """A circular obstacle (continuous_tools.py:468-487) as the 64-gon on the circle whose first
    vertex is at angle 0, counter-clockwise.  shapely's default ``buffer`` is a 64-gon too; the
    order of its vertices and their last digits are not claimed to be the same."""
    k = np.arange(64)
    ang = 2.0 * np.pi * k / 64.0
    c = np.stack([location[0] + radius * np.cos(ang), location[1] + radius * np.sin(ang)], axis=1)
    return Polygon(c)


def make_triangle(location, width: float, height: float, base: float = 0.5,
                  orientation: float = 0.0) -> Polygon:
    """A triangular obstacle ABC (continuous_tools.py:490-525): base AB of length ``width``, C
    above the point ``base`` along it; the centroid is moved to ``location``, then the triangle is
    rotated by ``orientation`` degrees about the centre of its bounding box."""
    c = np.array([[0, 0], [width, 0], [width * base, height], [0, 0]], dtype=np.float64)
    centroid = c[:3].mean(axis=0)
    c = c + (np.array([location[0], location[1]], dtype=np.float64) - centroid)
    origin = ((c[:, 0].min() + c[:, 0].max()) / 2.0, (c[:, 1].min() + c[:, 1].max()) / 2.0)
    return Polygon(_rotate(c, orientation, origin))
