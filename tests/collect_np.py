"""CPU restatement of data_gen_scripts/generate_locomaze.py:102-176
(hliuson/ogbench) for the point agent with injected draws, on top of the
oracle (oracle/locomaze.py): the checker of the fused collector
(include/ogbx_collect.h).  Test infrastructure only.

The script cannot run here (no MuJoCo, no Gymnasium), so its text is restated:
the stitch BFS literally, the episode step as one teacher-forced function of
(state, goal, draws), and the collector's documented Philox counter layout."""

import math
from fractions import Fraction

import numpy as np

from oracle import locomaze as orc

UNIT, OFF = 4.0, 4.0
GOAL_TOL = 1.0  # maze.py:86, point agent
PERIOD = 10  # generate_locomaze.py:150
TAG_MAZE_COLLECT = 0x4D5A0005
DOM_NORMAL, DOM_PICK, DOM_GNOISE, DOM_DIR = 0x61, 0x62, 0x63, 0x64


def maze_name(env_name):
    return env_name.split('-')[1]


def cells_of(maze_map):
    """(all empty cells, vertex cells), generate_locomaze.py:68-93."""
    m = maze_map
    all_cells, vertex_cells = [], []
    for i in range(m.shape[0]):
        for j in range(m.shape[1]):
            if m[i, j] == 0:
                all_cells.append((i, j))
                if m[i - 1, j] == 0 and m[i + 1, j] == 0 and m[i, j - 1] == 1 and m[i, j + 1] == 1:
                    continue
                if m[i, j - 1] == 0 and m[i, j + 1] == 0 and m[i - 1, j] == 1 and m[i + 1, j] == 1:
                    continue
                vertex_cells.append((i, j))
    return all_cells, vertex_cells


def script_adj_cells(maze_map, init_ij):
    """generate_locomaze.py:111-133, transcribed."""
    adj_cells = []
    adj_steps = 4
    bfs_map = maze_map.copy()
    for i in range(bfs_map.shape[0]):
        for j in range(bfs_map.shape[1]):
            bfs_map[i][j] = -1
    bfs_map[init_ij[0], init_ij[1]] = 0
    queue = [init_ij]
    while len(queue) > 0:
        i, j = queue.pop(0)
        for di, dj in [(-1, 0), (0, -1), (1, 0), (0, 1)]:
            ni, nj = i + di, j + dj
            if (
                0 <= ni < bfs_map.shape[0]
                and 0 <= nj < bfs_map.shape[1]
                and maze_map[ni, nj] == 0
                and bfs_map[ni, nj] == -1
            ):
                bfs_map[ni][nj] = bfs_map[i][j] + 1
                queue.append((ni, nj))
                if bfs_map[ni][nj] == adj_steps:
                    adj_cells.append((ni, nj))
    return adj_cells


def bfs_distances(maze_map, init_ij):
    """Plain BFS distances from init_ij over empty cells (-1 unreachable)."""
    d = np.full(maze_map.shape, -1, np.int64)
    d[init_ij] = 0
    frontier = [tuple(init_ij)]
    while frontier:
        nxt = []
        for i, j in frontier:
            for ni, nj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                if 0 <= ni < d.shape[0] and 0 <= nj < d.shape[1] and maze_map[ni, nj] == 0 and d[ni, nj] == -1:
                    d[ni, nj] = d[i, j] + 1
                    nxt.append((ni, nj))
        frontier = nxt
    return d


def ij_to_xy(ij):
    ij = np.asarray(ij)
    return np.stack([ij[..., 1] * UNIT - OFF, ij[..., 0] * UNIT - OFF], -1)


def fma_norm(vx, vy):
    """sqrt(fma(vy, vy, vx * vx)): np.linalg.norm of a pair through BLAS ddot."""
    vx, vy = float(vx), float(vy)
    return math.sqrt(float(Fraction(vy) * Fraction(vy) + Fraction(vx * vx)))


def explore_dirs(d):
    """generate_locomaze.py:151-152 for raw standard normals d [..., 2]."""
    d = np.asarray(d, np.float64)
    out = np.empty_like(d)
    for idx in np.ndindex(d.shape[:-1]):
        den = fma_norm(d[idx][0], d[idx][1]) + 1e-6
        out[idx] = d[idx] / den
    return out


def explore_actions(d, normal):
    """The explore action of every step: d [ceil(T / 10), N, 2] raw normals,
    normal [T, N, 2] finished N(0, noise) samples (generate_locomaze.py:148-166)."""
    dirs = explore_dirs(d)
    T = normal.shape[0]
    return np.clip(dirs[np.arange(T) // PERIOD] + normal, -1, 1)


def success_of(xy, goal):
    """compute_success (maze.py:486-490) with the fma norm, per row."""
    xy, goal = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(goal, np.float64).reshape(-1, 2)
    return np.array([fma_norm(a[0] - b[0], a[1] - b[1]) <= GOAL_TOL for a, b in zip(xy, goal)])


def new_goals(cells, pick, noise):
    """set_goal (maze.py:492-497) with add_noise: ij_to_xy + r * unit / 4."""
    xy = ij_to_xy(np.asarray(cells)[pick])
    return xy + np.asarray(noise) * UNIT / 4.0


# ------------------------------------------------------------ Philox layout
def u01_from(hi, lo):
    return float(((int(hi) << 32) | int(lo)) >> 11) * 2.0 ** -53


def bounded_u32(w, n):
    return (int(w) * int(n)) >> 32


def collect_key(seed):
    return orc.philox_key(seed, TAG_MAZE_COLLECT)


def _words(seed, g, c1, domain):
    k0, k1 = collect_key(seed)
    return orc.philox4x32([g & 0xFFFFFFFF, c1, domain, g >> 32], k0, k1)


def _box_muller(w):
    u1, u2 = 1.0 - u01_from(w[0], w[1]), u01_from(w[2], w[3])
    r, a = math.sqrt(-2.0 * math.log(u1)), 6.283185307179586 * u2
    return r * math.cos(a), r * math.sin(a)


def action_normal(seed, g, t, noise):
    """The step's N(0, noise) pair (to libm's rounding of log / cos / sin)."""
    c, s = _box_muller(_words(seed, g, t, DOM_NORMAL))
    return 0.0 + noise * c, 0.0 + noise * s


def explore_normal(seed, g, period):
    return _box_muller(_words(seed, g, period, DOM_DIR))


def goal_pick(seed, g, t, n_cells):
    return bounded_u32(_words(seed, g, t, DOM_PICK)[0], n_cells)


def goal_noise(seed, g, t):
    w = _words(seed, g, t, DOM_GNOISE)
    return -1.0 + 2.0 * u01_from(w[0], w[1]), -1.0 + 2.0 * u01_from(w[2], w[3])
