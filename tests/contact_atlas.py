"""Contact-regime atlas of the pointmaze contact step -- TEST INFRASTRUCTURE.

Deterministic builders of sphere centres, one per regime of the contact step
(``ogbench_amd/csrc/point_contact.h``: lean loop, full-loop redo, generic
collider, impedance band, corner slot, flag thresholds), built from the maze
map alone (``oracle.locomaze.tables``) with fixed seeds.  Random draws over a
free cell land in the impedance band (|dist| < 1 mm), on a cell edge or within
an ulp of the radius only by luck; here every such state is placed by hand.
tests/test_contact_atlas_cpu.py certifies that each class holds what its name
says (with ``mjmodel_np.contacts``) and that the oracle equals the enumeration
model on it; tests/test_contact_atlas_gpu.py holds the kernels to both.

Geometry: cell (i, j) has its centre at (j*4 - 4, i*4 - 4) and half size 2, a
wall cell is a box of that size, the sphere's radius is 0.7.  A site is a free
cell with an orientation: (sj, si) are the signs of the x and y directions
towards the walls in question.

Classes (each builder returns float64 qpos [n, 2]):
  face           one wall face at every BAND and DEEP depth, off the cell's axis
  outer_corner   free sides, wall diagonal: centre 0.7 - d from the box corner
  inner_corner   walls on both sides (and diagonal), depths (dx, dy) with dx != dy
  edge_wall_end  beside an outer corner, either side of (and on) the cell edge
  on_edge_face   centre exactly on the edge between two free cells, wall face
                 on the other axis
  rest           oracle trajectories settling into a wall, zero or small action
                 (states after REST_STEPS steps)
  flag_face      face distance within 6 ulp of the radius
  flag_corner    corner distance 0.7 (1 + k 2^-53), k in -6..6
  in_wall_cell   centre inside a wall cell
  in_wall_corner centre inside a wall cell, 0.7 - d from a corner where four
                 wall cells meet: its own box, both side boxes and the diagonal
                 one touch (the generic collider's four-contact regime)
  off_map        centre outside the map
"""

import functools
import math

import numpy as np

import mjmodel_np as mj
from oracle import locomaze as orc

MAZES = ('medium', 'large', 'giant')
RADIUS, HALF, UNIT, OFFSET = 0.7, 2.0, 4.0, 4.0
BAND = (1e-6, 1e-5, 1e-4, 2.5e-4, 5e-4, 7.5e-4, 9.99e-4)
DEEP = (0.002, 0.05, 0.15, 0.3, 0.45, 0.6)
EDGE_E = (-1e-3, -1e-9, 0.0, 1e-9, 1e-3, 0.1)
EDGE_PEN = (5e-4, 0.05, 0.3)
REST_STEPS = (1, 2, 3, 5, 8, 12, 20, 30, 45)
REST_PRESS = (0.01, 0.001)  # magnitudes of the constant action pressed into the wall
FLAG_K = tuple(range(-6, 7))
FLAG_PER_K = 154  # 13 * 154 = 2,002 states per flag class and maze
MODEL_CLASSES = ('face', 'outer_corner', 'inner_corner', 'edge_wall_end', 'on_edge_face', 'rest')
ORACLE_ONLY = ('flag_face', 'flag_corner', 'in_wall_cell', 'in_wall_corner', 'off_map')
CLASSES = MODEL_CLASSES + ORACLE_ONLY
# States per class and maze sent to the enumeration model (it costs 2^(4 + 4
# walls) pieces per stage: ~25 ms a state with two walls, ~0.5 s with three).
# The caps bound cost only; the class minima of test_contact_atlas_cpu.py are
# asserted on the capped subsets where they concern the model.
# in_wall_corner needs a 2 x 2 block of wall cells: pointmaze-large has none
# (test_in_wall_corner_touches_four_boxes checks this list against the maps)
IN_WALL_CORNER_MAZES = ('medium', 'giant')
MODEL_CAP = 32
MODEL_ALL = ('edge_wall_end',)  # one wall each, and the continuity check needs every triple
# Three-wall states: the issue's "at least 15" and "at most 24" are read as
# totals over the three mazes (the enumeration takes 0.2-1 s a state): 5 of
# inner_corner and up to 2 of rest per maze, so 15 to 21 in all, 15 of them
# inner_corner (test_model_subsets_keep_the_minima).
MODEL_CAP3 = dict(inner_corner=5, rest=2)


@functools.lru_cache(maxsize=None)
def maze_map(maze):
    return orc.tables(maze)[0]


@functools.lru_cache(maxsize=None)
def boxes(maze):
    return mj.wall_boxes(maze_map(maze))


def centre(i, j):
    return np.array([j * UNIT - OFFSET, i * UNIT - OFFSET])


@functools.lru_cache(maxsize=None)
def sites(maze):
    """Sites of the map by kind, each list sorted.
    face: (i, j, axis, s) wall on the s side of axis (0: x, 1: y);
    outer / inner: (i, j, si, sj); on_edge: (i, j, axis, se, sw) free cell on
    the se side of axis, wall on the sw side of the other axis; wall_corner:
    (i, j, si, sj) WALL cell whose two side cells and diagonal cell are walls."""
    mp = maze_map(maze)
    H, W = mp.shape

    def wall(i, j):
        return 0 <= i < H and 0 <= j < W and mp[i, j] == 1

    def free(i, j):
        return 0 <= i < H and 0 <= j < W and mp[i, j] == 0

    out = dict(face=[], outer=[], inner=[], on_edge=[], wall_corner=[])
    for i, j in np.argwhere(mp == 1).tolist():
        for si in (-1, 1):
            for sj in (-1, 1):
                if wall(i, j + sj) and wall(i + si, j) and wall(i + si, j + sj):
                    out['wall_corner'].append((i, j, si, sj))
    for i, j in np.argwhere(mp == 0).tolist():
        for s in (-1, 1):
            if wall(i, j + s):
                out['face'].append((i, j, 0, s))
            if wall(i + s, j):
                out['face'].append((i, j, 1, s))
        for si in (-1, 1):
            for sj in (-1, 1):
                if free(i, j + sj) and free(i + si, j) and wall(i + si, j + sj):
                    out['outer'].append((i, j, si, sj))
                if wall(i, j + sj) and wall(i + si, j) and wall(i + si, j + sj):
                    out['inner'].append((i, j, si, sj))
        for se in (-1, 1):
            for sw in (-1, 1):
                if free(i, j + se) and wall(i + sw, j):
                    out['on_edge'].append((i, j, 0, se, sw))
                if free(i + se, j) and wall(i, j + sw):
                    out['on_edge'].append((i, j, 1, se, sw))
    return out


def _pick(items, per, rng):
    """`per` items of every orientation (everything after the cell), in order."""
    groups = {}
    for it in items:
        groups.setdefault(it[2:], []).append(it)
    out = []
    for key in sorted(groups):
        g = groups[key]
        out += [g[k] for k in sorted(rng.choice(len(g), size=min(per, len(g)), replace=False).tolist())]
    return out


def _seed(maze, salt):
    return sum(map(ord, maze)) * 131 + salt


def _axis_point(c, axis, along, across):
    """Cell centre c plus `along` on axis and `across` on the other one."""
    d = np.array([along, across]) if axis == 0 else np.array([across, along])
    return c + d


@functools.lru_cache(maxsize=None)
def face(maze):
    rng = np.random.RandomState(_seed(maze, 1))
    out = []
    for i, j, axis, s in _pick(sites(maze)['face'], 2, rng):
        for d in BAND + DEEP:
            # off the axis by 0.05..1.2: no other box within the radius
            t = rng.uniform(0.05, 1.2) * rng.choice([-1.0, 1.0])
            out.append(_axis_point(centre(i, j), axis, s * (HALF - RADIUS + d), t))
    return np.array(out)


def _outer_point(i, j, si, sj, r, theta):
    corner = centre(i, j) + HALF * np.array([sj, si])
    return corner - r * np.array([sj * math.cos(theta), si * math.sin(theta)])


@functools.lru_cache(maxsize=None)
def outer_corner(maze):
    rng = np.random.RandomState(_seed(maze, 2))
    out = []
    for i, j, si, sj in _pick(sites(maze)['outer'], 1, rng):
        for d in BAND + DEEP:
            for theta in (0.03, math.pi / 2 - 0.03, rng.uniform(0.1, math.pi / 2 - 0.1)):
                out.append(_outer_point(i, j, si, sj, RADIUS - d, theta))
    return np.array(out)


def _depth_pairs():
    pairs = [(a, b) for a in BAND for b in DEEP] + [(a, b) for a in DEEP for b in BAND]
    pairs += [(a, b) for a in BAND for b in BAND if a != b]
    pairs += [(a, b) for a in DEEP for b in DEEP if a != b]
    return pairs


@functools.lru_cache(maxsize=None)
def inner_corner(maze):
    rng = np.random.RandomState(_seed(maze, 3))
    out = []
    for i, j, si, sj in _pick(sites(maze)['inner'], 1, rng):
        for dx, dy in _depth_pairs():
            out.append(centre(i, j) + np.array([sj * (HALF - RADIUS + dx), si * (HALF - RADIUS + dy)]))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def edge_wall_end(maze):
    """Rows ordered (site, axis, pen, e): reshape to [-1, len(EDGE_PEN),
    len(EDGE_E), 2].  axis 0: x holds the penetration and y crosses the edge."""
    rng = np.random.RandomState(_seed(maze, 4))
    out = []
    for i, j, si, sj in _pick(sites(maze)['outer'], 1, rng):
        for axis in (0, 1):
            sa, sb = (sj, si) if axis == 0 else (si, sj)
            for pen in EDGE_PEN:
                for e in EDGE_E:
                    out.append(_axis_point(centre(i, j), axis, sa * (HALF - RADIUS + pen), sb * (HALF + e)))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def on_edge_face(maze):
    rng = np.random.RandomState(_seed(maze, 5))
    out = []
    for i, j, axis, se, sw in _pick(sites(maze)['on_edge'], 1, rng):
        for pen in EDGE_PEN:
            out.append(_axis_point(centre(i, j), axis, se * HALF, sw * (HALF - RADIUS + pen)))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _rest(maze):
    rng = np.random.RandomState(_seed(maze, 6))
    S = sites(maze)
    q0, press = [], []
    for i, j, axis, s in _pick(S['face'], 1, rng):
        for d in (0.3, 0.05):
            q0.append(_axis_point(centre(i, j), axis, s * (HALF - RADIUS + d), rng.uniform(-1.0, 1.0)))
            press.append(_axis_point(np.zeros(2), axis, float(s), 0.0))
    for i, j, si, sj in _pick(S['outer'], 1, rng):
        theta = rng.uniform(0.2, math.pi / 2 - 0.2)
        q0.append(_outer_point(i, j, si, sj, RADIUS - 0.3, theta))
        press.append(np.array([sj * math.cos(theta), si * math.sin(theta)]))
    for i, j, si, sj in _pick(S['inner'], 1, rng):
        for dx, dy in ((0.3, 0.05), (0.3, 0.45)):
            q0.append(centre(i, j) + np.array([sj * (HALF - RADIUS + dx), si * (HALF - RADIUS + dy)]))
            press.append(np.array([sj, si]) / math.sqrt(2.0))
    for i, j, axis, se, sw in _pick(S['on_edge'], 1, rng)[::2]:
        q0.append(_axis_point(centre(i, j), axis, se * HALF, sw * (HALF - RADIUS + 0.3)))
        press.append(_axis_point(np.zeros(2), axis, 0.0, float(sw)))
    q0, press = np.array(q0), np.array(press)  # press: unit vectors into the wall
    qs, ps = [], []
    for mag in (0.0,) + REST_PRESS:
        q = q0.copy()
        for t in range(1, max(REST_STEPS) + 1):
            q, _ = orc.physics(maze, q, mag * press)
            if t in REST_STEPS:
                qs.append(q.copy())
                ps.append((mag or REST_PRESS[0]) * press)
    return np.concatenate(qs), np.concatenate(ps)


def rest(maze):
    return _rest(maze)[0]


def rest_press(maze):
    """Per state of rest(maze): the action into its wall that its trajectory
    held (REST_PRESS[0] for the zero-action trajectories)."""
    return _rest(maze)[1]


def _step_ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, math.copysign(np.inf, k))
    return x


@functools.lru_cache(maxsize=None)
def flag_face(maze):
    rng = np.random.RandomState(_seed(maze, 7))
    S = sites(maze)['face']
    out = []
    for k in FLAG_K:
        for n in range(FLAG_PER_K):
            i, j, axis, s = S[rng.randint(len(S))]
            c = centre(i, j)
            # the radius away from the face, then k ulp of that coordinate further away
            x = _step_ulps((c[axis] + s * HALF) - s * RADIUS, -s * k)
            out.append(_axis_point(np.array([0.0, 0.0]), axis, x, c[1 - axis] + rng.uniform(-1.2, 1.2)))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def flag_corner(maze):
    rng = np.random.RandomState(_seed(maze, 8))
    S = sites(maze)['outer']
    out = []
    for k in FLAG_K:
        for n in range(FLAG_PER_K):
            i, j, si, sj = S[rng.randint(len(S))]
            out.append(_outer_point(i, j, si, sj, RADIUS * (1.0 + k * 2.0 ** -53),
                                    rng.uniform(0.02, math.pi / 2 - 0.02)))
    return np.array(out)


def in_wall_cell(maze, n=480, seed=None):
    """Centres uniform over the wall cells of the map."""
    rng = np.random.RandomState(_seed(maze, 9) if seed is None else seed)
    wall_cells = np.argwhere(maze_map(maze) == 1)
    wc = wall_cells[rng.randint(len(wall_cells), size=n)]
    return np.stack([wc[:, 1] * UNIT - OFFSET + rng.uniform(-HALF, HALF, n),
                     wc[:, 0] * UNIT - OFFSET + rng.uniform(-HALF, HALF, n)], 1)


@functools.lru_cache(maxsize=None)
def in_wall_corner(maze):
    """Rows ordered (site, depth, angle).  The centre lies in wall cell (i, j)
    at distance RADIUS - d from the corner it shares with its (sj, si) side
    and diagonal cells, all walls: the offsets from the corner are below the
    radius on both axes, so the own box (centre inside it, pushed out through
    the nearer side face), both side boxes (faces) and the diagonal box
    (corner, penetration d) touch.  Angles off pi/4: no tie between the own
    box's two nearest faces."""
    rng = np.random.RandomState(_seed(maze, 11))
    out = []
    for i, j, si, sj in _pick(sites(maze)['wall_corner'], 1, rng):
        corner = centre(i, j) + HALF * np.array([sj, si])
        for d in BAND + DEEP:
            r = RADIUS - d
            for theta in (0.15, math.pi / 2 - 0.15, rng.uniform(0.25, math.pi / 4 - 0.1),
                          rng.uniform(math.pi / 4 + 0.1, math.pi / 2 - 0.25)):
                out.append(corner - r * np.array([sj * math.cos(theta), si * math.sin(theta)]))
    return np.array(out).reshape(-1, 2)  # [0, 2] in a maze without such a corner


def touching_boxes(maze, q):
    """Wall boxes within the radius of centre q (a box that holds the centre
    counts: distance 0), by plain geometry over every wall cell of the map."""
    n = 0
    for i, j in np.argwhere(maze_map(maze) == 1):
        p = q - centre(i, j)
        t = np.clip(p, -HALF, HALF) - p
        n += math.hypot(t[0], t[1]) - RADIUS <= 0.0
    return int(n)


@functools.lru_cache(maxsize=None)
def off_map(maze):
    """Outside every cell of the map: within the radius of the outer wall's
    outer faces and corners (contact), at the radius, beyond it and far away."""
    H, W = maze_map(maze).shape
    x0, x1, y0, y1 = -OFFSET - HALF, W * UNIT - OFFSET - HALF, -OFFSET - HALF, H * UNIT - OFFSET - HALF
    out = []
    for d in (5e-4, 0.3, 0.6999, RADIUS, 0.7001, 1.5):
        out += [[x0 - d, 1.3], [x1 + d, y1 - 3.1], [2.7, y0 - d], [x0 + 5.0, y1 + d]]
    for d in (0.2, 0.45, 0.6):  # outside the four outer corners
        out += [[x0 - d, y0 - d], [x1 + d, y0 - 0.5 * d], [x0 - 0.5 * d, y1 + d], [x1 + d, y1 + d]]
    out += [[x0 - UNIT, y0 - UNIT], [x0 - 100.0, 3.0], [7.0, y1 + 1e3], [-1e6, 1e6], [x1 + 2.0 * UNIT, 0.0]]
    return np.array(out)


BUILDERS = dict(face=face, outer_corner=outer_corner, inner_corner=inner_corner, edge_wall_end=edge_wall_end,
                on_edge_face=on_edge_face, rest=rest, flag_face=flag_face, flag_corner=flag_corner,
                in_wall_cell=in_wall_cell, in_wall_corner=in_wall_corner, off_map=off_map)


def states(maze, label):
    q = BUILDERS[label](maze)
    q.setflags(write=False)  # shared between tests
    return q


def atlas(maze):
    """label -> qpos [n, 2] for every class, in the order of CLASSES."""
    return {label: states(maze, label) for label in CLASSES}


def wall_contacts(maze, q):
    """Wall contacts of mjmodel_np.contacts (the floor left out)."""
    return mj.contacts(q, boxes(maze))[1:]


@functools.lru_cache(maxsize=None)
def model_subset(maze, label):
    """Indices into states(maze, label) of the states sent to the enumeration
    model: evenly spread, at most MODEL_CAP with up to two wall contacts and
    MODEL_CAP3[label] with three.  Of rest, three quarters of the cap go to
    the states inside the impedance band (the class is about them)."""
    q = states(maze, label)
    cons = [wall_contacts(maze, x) for x in q]
    nw = np.array([len(c) for c in cons])

    def spread(idx, cap):
        if label in MODEL_ALL:
            return idx
        return idx if len(idx) <= cap else idx[np.unique(np.linspace(0, len(idx) - 1, cap).round().astype(int))]

    if label == 'rest':
        pen = np.array([min(abs(d) for d, _, _ in c) for c in cons])
        floor, band = pen < 1e-9, (pen >= 1e-9) & (pen < 1e-3)  # resting at a few ulp; the band above that
        return np.sort(np.concatenate([spread(np.flatnonzero((nw <= 2) & floor), MODEL_CAP // 4),
                                       spread(np.flatnonzero((nw <= 2) & band), MODEL_CAP // 2),
                                       spread(np.flatnonzero((nw <= 2) & ~floor & ~band), MODEL_CAP // 4),
                                       spread(np.flatnonzero(nw >= 3), MODEL_CAP3[label])]))
    return np.sort(np.concatenate([spread(np.flatnonzero(nw <= 2), MODEL_CAP),
                                   spread(np.flatnonzero(nw >= 3), MODEL_CAP3.get(label, 0))]))


@functools.lru_cache(maxsize=None)
def model_answers(maze, label):
    """mjmodel_np.point_step on model_subset(maze, label): qpos [m, 2].
    Computed once per process and shared by the tests that need it."""
    q = states(maze, label)[model_subset(maze, label)]
    out = np.array([mj.point_step(x, boxes(maze))[0] for x in q])
    out.setflags(write=False)
    return out
