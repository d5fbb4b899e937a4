"""tests/online_visual_np.py -- TEST INFRASTRUCTURE ONLY.

NumPy restatement of visual batches over the episode ring
(include/ogbx_online_visual.h; ``GCReplayBuffer`` / ``HGCReplayBuffer`` with
``frame_stack`` / ``p_aug``) over ``tests/online_np.OnlineNp``.  The plain
batch is ``OnlineNp.sample`` / ``online_hgc_np.hgc_sample``; the image keys
are rebuilt here from the ring's own tables:

  stack  channel block j (0..F-1) of a selector row at step t of env e is the
         ``observations`` frame at step max(t - (F-1-j), s0), s0 the earliest
         step among t - (F-1) .. t that is live (>= S - L) and whose ep_seq
         equals the row's
  next   blocks 1 .. F-1 of the stacked observations, then the ring's own
         ``next_observations`` row
  crop   tests/visual_np.crop (the clamp formula), after stacking

``stack_flat_snapshot`` is the second form the CPU tests hold the first
against: the reference's initial_locs rule over the snapshot's terminals.
"""

import numpy as np

import online_hgc_np as ohn
import online_np as onp
import visual_np as vnp

PADDING = vnp.PADDING

# the configs of tests/golden/online_visual_golden.npz: two of online_golden's
# and online_hgc_golden's hlow with subgoal_steps = 2 (its other step keys
# removed), each with frame_stack 3 and p_aug 1
F_GOLD = 3
GOLDEN_CONFIGS = {
    'geom': dict(onp.GOLDEN_CONFIGS['geom_neg'], frame_stack=F_GOLD, p_aug=1.0),
    'unif': dict(onp.GOLDEN_CONFIGS['unif_pos'], frame_stack=F_GOLD, p_aug=1.0),
    'hlow': dict({k: v for k, v in ohn.GOLDEN_CONFIGS['hlow'].items()
                  if k not in ('value_subgoal_steps', 'actor_subgoal_steps', 'low_subgoal_steps')},
                 subgoal_steps=2, frame_stack=F_GOLD, p_aug=1.0),
}
HGC = {'geom': False, 'unif': False, 'hlow': True}

# the designed history of the fixture: make_golden_online's N, T, steps and done pattern
N, T, STEPS, B = 5, 6, 17, 64
SNAPS = (3, 6, 11, 17)
DONE_AT = {0: (2, 3, 9, 14), 1: (3, 10), 2: (0, 7, 8, 15), 3: (6, 12), 4: ()}
FRAME = (6, 5, 2)
EXAMPLE = dict(observations=np.zeros(FRAME, np.uint8), actions=np.zeros(2, np.float32),
               next_observations=np.zeros(FRAME, np.uint8))


def frame_of(e, t, shape=FRAME):
    """The uint8 frame of env e at episode-time t: every pixel encodes
    (env, step) and its own position, so no two frames and no two pixels of a
    frame's row are equal."""
    h, w, c = shape
    pos = np.arange(h * w * c).reshape(shape)
    return ((37 * e + 11 * t + 3 * pos + (pos // (w * c))) % 251).astype(np.uint8)


def history():
    """(rows [STEPS, N, ...], done [STEPS, N]) with
    next_observations[t] == observations[t + 1] inside an episode: an env's
    frame counter runs on through a done (the final observation) and the next
    episode starts two counts later (the reset observation)."""
    done = np.zeros((STEPS, N), bool)
    for e, steps in DONE_AT.items():
        done[list(steps), e] = True
    obs = np.zeros((STEPS, N) + FRAME, np.uint8)
    nxt = np.zeros((STEPS, N) + FRAME, np.uint8)
    for e in range(N):
        c = 0
        for t in range(STEPS):
            obs[t, e], nxt[t, e] = frame_of(e, c), frame_of(e, c + 1)
            c += 2 if done[t, e] else 1
    rng = np.random.RandomState(21)
    return dict(observations=obs, actions=rng.randint(-9, 10, (STEPS, N, 2)).astype(np.float32),
                next_observations=nxt), done


# ------------------------------------------------------------------- the stack
def stack_flat(ring, flat, F):
    """[B, F] flat snapshot rows of the F channel blocks of the selector rows
    ``flat``, from the ring's ep_seq and the liveness bound."""
    flat = np.asarray(flat, np.int64)
    S, L, T_ = ring.S, ring.L, ring.T
    e, k = ring.split(flat)
    t = S - L + k
    out = np.empty((len(flat), F), np.int64)
    for b in range(len(flat)):
        own = ring.ep_seq[t[b] % T_, e[b]]
        s0 = t[b]
        for i in range(1, F):
            tp = t[b] - i
            if tp < S - L or ring.ep_seq[tp % T_, e[b]] != own:
                break
            s0 = tp
        for j in range(F):
            out[b, j] = e[b] * L + (max(t[b] - (F - 1 - j), s0) - (S - L))
    return out


def stack_flat_snapshot(ring, flat, F):
    """The same rows by get_stacked_observations' rule (datasets.py:359-366)
    over the snapshot's terminals."""
    term = ring.snapshot()['terminals']
    locs = np.flatnonzero(term > 0)
    initial = np.concatenate([[0], locs[:-1] + 1])
    flat = np.asarray(flat, np.int64)
    first = initial[np.searchsorted(initial, flat, side='right') - 1]
    return np.stack([np.maximum(flat - i, first) for i in reversed(range(F))], axis=1)


def stacked(ring, flat, F):
    """observations[flat] with F frames joined on the last axis."""
    src = stack_flat(ring, flat, F)
    obs = ring.cols['observations']
    return np.concatenate([obs[ring.phys(src[:, j])] for j in range(F)], axis=-1)


def stacked_next(ring, flat, F):
    """The stacked next_observations of a ring that stores its own."""
    d = ring.cols['observations'].shape[-1]
    own = ring.cols['next_observations'][ring.phys(flat)]
    return np.concatenate([stacked(ring, flat, F)[..., d:], own], axis=-1)


# ------------------------------------------------------------------ the sample
def selectors(ring, cfg, ix, hgc):
    """selector -> flat rows (ogbx_online_hgc_sample's numbering, no 1)."""
    if not hgc:
        return {0: ix['idxs'], 2: ix['vg'], 3: ix['ag']}
    tend = vnp.traj_end(ring.snapshot()['terminals'])
    sel = vnp.hgc_selectors(ix['idxs'], ix['hvg'], ix['hag'], ix['lvg'], tend, ring.L * ring.N, *vnp.hgc_steps(cfg))
    del sel[1]
    return sel


def sample(ring, cfg, draws, crop_from=None, hgc=False, idxs=None):
    """(batch, indices) of one visual sample: what ``GCReplayBuffer.sample`` /
    ``HGCReplayBuffer.sample`` return under ``cfg`` with the injected draws;
    crop_from [B, 2] when the call's coin came up, else None."""
    F = cfg.get('frame_stack')
    plain_cfg = dict(cfg, frame_stack=None, p_aug=None)
    if hgc:
        assert idxs is None
        out, ix = ohn.hgc_sample(ring, plain_cfg, draws)
        keys, goal_keys, uncropped = vnp.HGC_KEYS, vnp.HGC_GOAL_KEYS, vnp.HGC_UNCROPPED
    else:
        out, i, vg, ag = ring.sample(plain_cfg, draws, idxs)
        ix = dict(idxs=i, vg=vg, ag=ag)
        keys, goal_keys, uncropped = vnp.GC_KEYS, vnp.GC_GOAL_KEYS, ()
    sel = selectors(ring, cfg, ix, hgc)
    made = {}  # selector -> stacked observations: aliases of the plain batch stay aliases of one array
    for key in out:
        if key not in keys or ('oracle_reps' in ring.cols and key in goal_keys):
            continue
        if key == 'next_observations':
            v = stacked_next(ring, ix['idxs'], F) if F is not None else out[key]
        elif F is not None:
            s = keys[key]
            if s not in made:
                made[s] = stacked(ring, sel[s], F)
            v = made[s]
        else:
            v = out[key]
        if crop_from is not None and v.ndim == 4 and key not in uncropped:
            v = vnp.crop(v, crop_from)
        out[key] = v
    return out, ix


def crop_draws(rng, B):
    return rng.randint(0, 2 * PADDING + 1, (B, 2)).astype(np.int64)
