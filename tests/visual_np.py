"""NumPy restatement of the visual batch semantics (frame stack and random
crop) of GCDataset / HGCDataset, written from the closed forms, not from the
reference's code paths.  Test infrastructure: the CPU tests check it against
the reference's recorded batches (tests/golden/visual_golden.npz), the GPU
tests check the HIP kernel against it.

Closed forms
  stack  channel block j (0..F-1) of row r is the frame at row
         max(r - (F-1-j), start(r)), start(r) the first row of r's trajectory;
         row r-s is in r's trajectory iff r-s >= 0 and
         traj_end[r-s] == traj_end[r]
  crop   out[y, x, :] = img[clamp(y + cy - p, 0, H-1), clamp(x + cx - p, 0, W-1), :]
"""

import numpy as np

PADDING = 3

GC_KEYS = {'observations': 0, 'next_observations': 1, 'value_goals': 2, 'actor_goals': 3}
GC_GOAL_KEYS = ('value_goals', 'actor_goals')
# HGC key -> selector (numbering of ogbx_hgc_sample)
HGC_KEYS = {
    'observations': 0, 'next_observations': 1, 'high_value_reps': 0, 'high_value_goals': 2, 'value_goals': 2,
    'high_value_actions': 4, 'high_value_next_observations': 4, 'low_value_next_observations': 5,
    'low_value_goals': 6, 'high_actor_goals': 3, 'high_actor_actions': 7, 'high_actor_targets': 7,
    'high_actor_next_observations': 7, 'low_actor_goals': 8, 'low_actor_goal_observations': 8,
    'low_actor_next_observations': 9,
}
HGC_GOAL_KEYS = ('high_value_goals', 'value_goals', 'high_value_actions', 'low_value_goals', 'high_actor_goals',
                 'high_actor_actions', 'high_actor_targets', 'low_actor_goals')
HGC_UNCROPPED = ('high_value_reps', 'low_value_goals')


def traj_end(terminals):
    """Trajectory end row of every row ('terminals' marks each trajectory's last row)."""
    locs = np.nonzero(np.asarray(terminals) > 0)[0]
    return locs[np.searchsorted(locs, np.arange(len(terminals)))]


def stack_rows(rows, tend, F):
    """[B, F] source rows of the F channel blocks of the selector rows."""
    rows = np.asarray(rows, np.int64)
    out = np.empty((len(rows), F), np.int64)
    for b, r in enumerate(rows):
        start = r
        while start - 1 >= 0 and r - (start - 1) < F and tend[start - 1] == tend[r]:
            start -= 1
        for j in range(F):
            out[b, j] = max(r - (F - 1 - j), start)
    return out


def stacked(frames, rows, tend, F):
    """frames[rows] with F frames stacked on the last axis."""
    src = stack_rows(rows, tend, F)
    return np.concatenate([frames[src[:, j]] for j in range(F)], axis=-1)


def crop(imgs, crop_from, p=PADDING):
    """The random crop with edge padding p of a [B, H, W, C] batch."""
    B, H, W = imgs.shape[:3]
    cf = np.asarray(crop_from, np.int64)
    ys = np.clip(np.arange(H)[None, :] + cf[:, :1] - p, 0, H - 1)  # [B, H]
    xs = np.clip(np.arange(W)[None, :] + cf[:, 1:2] - p, 0, W - 1)  # [B, W]
    return imgs[np.arange(B)[:, None, None], ys[:, :, None], xs[:, None, :]]


def high_next(idx, fin, goal, K):
    st = np.minimum(K, fin - idx)
    diff = goal - idx
    st = np.where((0 <= diff) & (diff < st), diff, st)
    return idx + st


def gc_selectors(idxs, value_goals, actor_goals, R):
    idxs = np.asarray(idxs, np.int64)
    return {0: idxs, 1: np.minimum(idxs + 1, R - 1), 2: np.asarray(value_goals), 3: np.asarray(actor_goals)}


def hgc_selectors(idxs, hvg, hag, lvg, tend, R, k_value, k_low, k_actor):
    idxs = np.asarray(idxs, np.int64)
    fin = tend[idxs]
    return {
        0: idxs, 1: np.minimum(idxs + 1, R - 1), 2: np.asarray(hvg), 3: np.asarray(hag),
        4: high_next(idxs, fin, hvg, k_value), 5: high_next(idxs, fin, hvg, k_low), 6: lvg,
        7: high_next(idxs, fin, hag, k_actor), 8: np.minimum(idxs + k_actor, fin),
        9: high_next(idxs, fin, hag, k_low),
    }


def visual_batch(dataset, selectors, frame_stack, crop_from, hgc=False, has_low=True):
    """The image keys of a batch.  dataset: dict of arrays with 'observations'
    and 'terminals' (and 'next_observations' when not compact); selectors: as
    gc_selectors / hgc_selectors return; crop_from: [B, 2] or None (the call
    did not crop).  Goal-type keys are left out when 'oracle_reps' exists."""
    obs = dataset['observations']
    tend = traj_end(dataset['terminals'])
    keys = dict(HGC_KEYS if hgc else GC_KEYS)
    goal_keys = HGC_GOAL_KEYS if hgc else GC_GOAL_KEYS
    uncropped = HGC_UNCROPPED if hgc else ()
    if hgc and not has_low:
        keys.pop('low_value_goals')
    out = {}
    for k, sel in keys.items():
        if 'oracle_reps' in dataset and k in goal_keys:
            continue
        rows, frames = selectors[sel], obs
        if k == 'next_observations' and 'next_observations' in dataset:
            assert frame_stack is None
            rows, frames = selectors[0], dataset['next_observations']
        v = stacked(frames, rows, tend, frame_stack) if frame_stack is not None else frames[rows]
        if crop_from is not None and v.ndim == 4 and k not in uncropped:
            v = crop(v, crop_from)
        out[k] = v
    return out


# ------------------------------------------------------------------ the fixture
# tests/golden/visual_golden.npz (make_golden_visual.py): the configs it ran
GC_CFG = dict(discount=0.99, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3,
              value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0,
              actor_geom_sample=False, gc_negative=True, p_aug=1.0, frame_stack=3)
HGC_CFG = dict(discount=0.97, value_p_curgoal=0.3, value_p_trajgoal=0.4, value_p_randomgoal=0.3,
               value_geom_sample=False, actor_p_curgoal=0.2, actor_p_trajgoal=0.5, actor_p_randomgoal=0.3,
               actor_geom_sample=True, gc_negative=False, p_aug=1.0, frame_stack=3, subgoal_steps=6,
               value_subgoal_steps=7, actor_subgoal_steps=4, low_subgoal_steps=3, low_discount=0.95)
# case -> (config, hierarchical, evaluation)
CASES = {
    'A': (GC_CFG, False, False), 'B': (GC_CFG, False, False), 'C': (GC_CFG, False, False),
    'D': (GC_CFG, False, True), 'E': (HGC_CFG, True, False), 'F': (dict(GC_CFG, frame_stack=None), False, False),
}


def fixture_case(gold, case):
    """(dataset, draws incl. 'crop_from' when the call cropped, expected batch)."""
    def part(tag):
        p = f'{case}_{tag}_'
        return {k[len(p):]: gold[k] for k in gold if k.startswith(p)}

    draws = part('draw')
    draws.pop('coin', None)
    return part('in'), draws, part('out')


def hgc_steps(cfg):
    high = cfg.get('high_subgoal_steps', cfg['subgoal_steps'])
    return (high if cfg.get('value_subgoal_steps') is None else cfg['value_subgoal_steps'],
            cfg.get('low_subgoal_steps', cfg['subgoal_steps']),
            high if cfg.get('actor_subgoal_steps') is None else cfg['actor_subgoal_steps'])
