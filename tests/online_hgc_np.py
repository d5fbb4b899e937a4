"""tests/online_hgc_np.py -- TEST INFRASTRUCTURE ONLY.

The hierarchical sample over the episode ring, restated: the snapshot of
``tests/online_np.OnlineNp`` (the ring's tables and unrolling) under
``oracle/gcdataset_np.hgc_sample`` (the restatement of the reference's
``HGCDataset.sample``), with the keys ``HGCReplayBuffer.sample`` returns, plus
the regime counts the tests must reach, taken from the model alone.
"""

import numpy as np

import online_np as onp
from oracle import gcdataset_np as gco

# the configs of tests/golden/online_hgc_golden.npz: make_golden_gc.HGC_CONFIGS
# with the subgoal steps shortened to a ring of 12 slots
GOLDEN_CONFIGS = {
    'hiql': dict(discount=0.99, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3,
                 value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0,
                 actor_geom_sample=False, gc_negative=True, p_aug=0.0, frame_stack=None, subgoal_steps=3),
    'hlow': dict(discount=0.97, value_p_curgoal=0.3, value_p_trajgoal=0.4, value_p_randomgoal=0.3,
                 value_geom_sample=False, actor_p_curgoal=0.2, actor_p_trajgoal=0.5, actor_p_randomgoal=0.3,
                 actor_geom_sample=True, gc_negative=False, p_aug=None, frame_stack=None, subgoal_steps=3,
                 value_subgoal_steps=4, actor_subgoal_steps=2, low_subgoal_steps=1, low_discount=0.95),
    'hcur': dict(discount=0.9, value_p_curgoal=1.0, value_p_trajgoal=0.0, value_p_randomgoal=0.0,
                 value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=0.5, actor_p_randomgoal=0.5,
                 actor_geom_sample=False, gc_negative=True, p_aug=None, frame_stack=None, subgoal_steps=2,
                 high_subgoal_steps=5, low_discount=0.9),
}

# the scripted history of the fixture
N, T, STEPS, B = 5, 12, 31, 64
SNAPS = (4, 12, 20, 31)
DONE_AT = {0: (2, 3, 9, 14, 27), 1: (5, 18, 29), 2: (0, 7, 8, 15, 22, 23), 3: (11, 24), 4: ()}
REGIMES = ('full_step', 'clip_end', 'clip_goal', 'goal_behind', 'zero_steps', 'open_episode', 'closed_episode',
           'wrapped_subgoal')


def value_steps(cfg):
    """The resolved value_subgoal_steps (HGCDataset.__init__)."""
    high = cfg.get('high_subgoal_steps', cfg['subgoal_steps'])
    return high if cfg.get('value_subgoal_steps') is None else cfg['value_subgoal_steps']


def hgc_sample(ring, cfg, draws):
    """(batch, indices) of one hierarchical sample over ``ring`` (an
    ``OnlineNp``): the batch holds the buffer's keys and the reference's
    hierarchical keys in the reference's order; indices are flat."""
    snap = ring.snapshot()
    out, ix = gco.hgc_sample(snap, cfg, draws)
    if 'terminals' not in ring.cols:
        del out['terminals']  # the snapshot's own column
    else:  # the buffer's own column holds what was inserted
        out['terminals'] = ring.cols['terminals'][ring.phys(ix['idxs'])]
    if ix['lvg'] is None:
        ix = dict(ix, lvg=ix['idxs'])
    return out, ix


def random_draws(rng, B, npick, low, max_geom=6):
    """Injected draws over a snapshot of npick rows (names as ogbx_hgc_draws)."""
    d = onp.random_draws(rng, B, npick, max_geom)
    if low:
        d['l_pick'] = rng.randint(0, npick, B).astype(np.int64)
        d['l_geom'] = rng.randint(1, max_geom + 1, B).astype(np.int64)
        d['l_u_traj'] = rng.rand(B)
        d['l_u_cur'] = rng.rand(B)
    return d


def _end(ring, ix):
    """(env, live offset, step, episode end step, open episode?) of flat rows."""
    e, k = ring.split(ix)
    steps = ring.S - ring.L + k
    end = ring.end_steps()[e, k]
    open_ep = ring.ep_seq[steps % ring.T, e] == ring.cur_seq[e]
    return e, k, steps, end, open_ep


def regimes(ring, idxs, hvg, steps_out, K):
    """Counts of the regimes of ``high_value_subgoal_steps`` (clipped step count
    ``steps_out`` for K = value_subgoal_steps), from the model alone."""
    ix, hvg, st = np.asarray(idxs), np.asarray(hvg), np.asarray(steps_out)
    e, k, steps, end, open_ep = _end(ring, ix)
    room = end - steps  # fin - idx
    diff = hvg - ix
    by_goal = (0 <= diff) & (diff < np.minimum(K, room))
    sub = ix + st
    return dict(
        full_step=int((st == K).sum()),
        clip_end=int((~by_goal & (room < K)).sum()),
        clip_goal=int(by_goal.sum()),
        goal_behind=int((diff < 0).sum()),
        zero_steps=int((st == 0).sum()),
        open_episode=int(open_ep.sum()),
        closed_episode=int((~open_ep).sum()),
        wrapped_subgoal=int((ring.phys(sub) < ring.phys(ix)).sum()),
    )


def gpu_regimes(ring, ix, draws, cfg, steps_out):
    """The regimes of the GPU coverage test: ``regimes`` with the clip by the
    episode end split into open / closed episodes, a random goal in another
    env, and a low value goal equal to idx (-1 without low value goals)."""
    idxs, hvg, lvg = ix['idxs'], ix['hvg'], ix['lvg']
    K = value_steps(cfg)
    r = regimes(ring, idxs, hvg, steps_out, K)
    e, k, steps, end, open_ep = _end(ring, idxs)
    room, diff = end - steps, hvg - idxs
    by_end = ~((0 <= diff) & (diff < np.minimum(K, room))) & (room < K)
    p_cur = cfg['value_p_curgoal']
    is_cur = draws['v_u_cur'] < p_cur
    is_traj = ~is_cur & (draws['v_u_traj'] < (cfg['value_p_trajgoal'] / (1 - p_cur) if p_cur != 1 else 0))
    ge, _ = ring.split(hvg)
    has_low = cfg.get('low_discount') is not None
    return dict(full_step=r['full_step'], clip_open=int((by_end & open_ep).sum()),
                clip_closed=int((by_end & ~open_ep).sum()), clip_goal=r['clip_goal'], goal_behind=r['goal_behind'],
                random_other_env=int((~is_cur & ~is_traj & (ge != e)).sum()), wrapped_subgoal=r['wrapped_subgoal'],
                low_goal_is_idx=int((lvg == idxs).sum()) if has_low else -1)
