"""The seeded near-wall batch of tests/test_maze_last_stage_gpu.py (and of
scripts/probe_last_stage.py): pointmaze-large envs resting against a face, in
an inner corner (two or three walls among the face, face and diagonal boxes of
a side) or at an outer corner (only the diagonal box is a wall), with float32
actions that push into those walls for K steps.

The point radius is 0.7 and a cell's half size 2, so an env touches a face
from an offset of 1.3 off its cell's centre; an action moves it by up to 0.2
before the contact test.
"""
import numpy as np

from oracle import locomaze as orc

MAZE, K, SEED = 'large', 8, 11


def _spots(mp):
    """(i, j, sx, sy, kind) of every free cell's sides: kind 0 a face (the x or the y box only), 1 an inner corner
    (both face boxes), 2 an outer corner (the diagonal box only)."""
    out = []
    for i, j in np.argwhere(mp == 0):
        for sx in (-1, 1):
            for sy in (-1, 1):
                fx, fy, fd = int(mp[i, j + sx]), int(mp[i + sy, j]), int(mp[i + sy, j + sx])
                if fx + fy == 1:
                    out.append((i, j, sx if fx else 0, sy if fy else 0, 0))
                elif fx + fy == 2:
                    out.append((i, j, sx, sy, 1))
                elif fd:
                    out.append((i, j, sx, sy, 2))
    return np.array(out)


def near_wall_batch(n):
    """qpos [n, 2] f64, actions [K, n, 2] f32 and the kind of each env (0 face, 1 inner corner, 2 outer corner).
    Env 0 is an inner corner, env 1 an outer corner and env 2 a face, whatever n draws."""
    rng = np.random.RandomState(SEED)
    mp, _ = orc.tables(MAZE)
    spots = _spots(mp)
    pick = spots[rng.randint(len(spots), size=max(n, 3))]
    for lane, kind in enumerate((1, 2, 0)):
        pick[lane] = spots[spots[:, 4] == kind][0]
    pick = pick[:n]
    m = len(pick)
    sx, sy, kind = pick[:, 2], pick[:, 3], pick[:, 4]
    # towards a wall: 1.15-1.6 off the centre (touching after the first action at the latest); an outer corner's env
    # sits on the diagonal of its corner point, 0.3-0.65 from it; a face's free axis anywhere in the cell's inner part
    off = rng.uniform(1.15, 1.6, (m, 2))
    free = rng.uniform(-1.0, 1.0, (m, 2))
    diag = 2.0 - rng.uniform(0.3, 0.65, m) / np.sqrt(2.0)
    ox = np.where(kind == 2, sx * diag, np.where(sx != 0, sx * off[:, 0], free[:, 0]))
    oy = np.where(kind == 2, sy * diag, np.where(sy != 0, sy * off[:, 1], free[:, 1]))
    q = np.stack([pick[:, 1] * 4.0 - 4.0 + ox, pick[:, 0] * 4.0 - 4.0 + oy], 1)
    # push into the walls on the walled axes (magnitude 0.5-1), anywhere on a face's free axis
    mag = rng.uniform(0.5, 1.0, (K, m, 2))
    anyw = rng.uniform(-1.0, 1.0, (K, m, 2))
    ax = np.where(sx != 0, sx * mag[:, :, 0], anyw[:, :, 0])
    ay = np.where(sy != 0, sy * mag[:, :, 1], anyw[:, :, 1])
    acts = np.stack([ax, ay], 2).astype(np.float32)
    return q, acts, kind


def oracle_run(q, acts, goal, elapsed, task, episode, seed):
    """The oracle's K steps (auto-reset on) from the batch, one step at a time: the outputs [K, n, ...] and the share
    of envs in wall contact at the start of each step (the oracle's contact flag, after the action's move)."""
    st = dict(qpos=q.copy(), goal=goal.copy(), elapsed=elapsed.copy(), task=task.copy(),
              episode=episode.view(np.uint32).copy(), opts=orc._opts())
    key = orc.philox_key(seed, orc.TAG_MAZE_RESET)
    rows, share = [], []
    for t in range(len(acts)):
        _, contact = orc.physics(MAZE, st['qpos'], acts[t])
        share.append(float(contact.mean()))
        rows.append(orc.step(MAZE, st, acts[t:t + 1], auto_reset=1, key=key))
    out = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    return out, np.array(share), st
