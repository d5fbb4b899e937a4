"""Golden fixtures for visual batches over the episode ring
(include/ogbx_online_visual.h; ``GCReplayBuffer`` / ``HGCReplayBuffer`` with
``frame_stack`` / ``p_aug``), from the reference's own ``GCDataset`` /
``HGCDataset`` (impls/utils/datasets.py).

Reuses make_golden_gc's loader of the reference modules and its recorder of
np.random draws, and make_golden_visual's NumPy stand-ins for the three jax
calls of the crop.  The history is make_golden_online's designed one -- N = 5
envs, T = 6 slots, 17 steps, its done pattern -- with uint8 6 x 5 x 2 frames
whose pixels encode (env, step) and ``next_observations[t] ==
observations[t + 1]`` inside an episode (tests/online_visual_np.history), kept
as plain per-env lists (tests/online_np.Brute: no ring, no table).  At steps
3, 6, 11 and 17 the live rows are laid out as a dataset and a batch of 64 is
put together from the reference's own pieces, since its ``sample`` refuses
``frame_stack`` on a dataset that stores ``next_observations``:

  the plain batch, the indices and their draws
      ``sample`` of a sampler without ``frame_stack`` over the snapshot, with
      ``augment`` replaced on the instance by the steps below (``sample`` calls
      it after its coin, with its own list of keys); the indices by the same
      calls in the same order under the same seed: ``get_random_idxs``,
      ``sample_goals``, ``compute_high_next_idxs``
  the stacked keys
      ``get_stacked_observations`` of a sampler with ``frame_stack`` and
      ``preprocess_frame_stack=False`` over the snapshot without
      ``next_observations``, at the index the plain batch shows for the key
      (asserted: the plain key equals the snapshot's observations there)
  next_observations
      the same function at u' + 1 over the compact unrolling of the snapshot:
      each episode's rows followed by one extra row holding its last
      ``next_observations``
  the crop
      the reference's ``augment`` with the keys ``sample`` passed; its
      ``randint`` is recorded as ``crop_from``

Saves arrays only (tests/golden/online_visual_golden.npz):

  in_<key> [17, 5, ...], done [17, 5], snap_steps     the history
  s<S>_<cfg>_draw_<name>     the recorded draws (names as ogbx_gc_draws /
                             ogbx_hgc_draws) and ``crop_from`` [64, 2]
  s<S>_<cfg>_out_<key>, s<S>_<cfg>_keys               the batch and its key order

Configs (tests/online_visual_np.GOLDEN_CONFIGS): GC with geometric and with
uniform trajectory goals, HGC with ``low_discount`` and ``subgoal_steps = 2``;
all with ``frame_stack = 3`` and ``p_aug = 1``.  ``counts`` are asserted >= 1
each: a stack clamped at an episode start, a stack clamped at the oldest live
row of an overwritten episode, a stack crossing the physical wrap from slot
T - 1 to slot 0, an episode of length 1, a goal row whose stack clamps, and
crop offsets of 0 and 6 on each axis.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_gc as gg  # noqa: E402
import make_golden_visual as gv  # noqa: E402
import online_np as onp  # noqa: E402
import online_visual_np as ovn  # noqa: E402

N, T, STEPS, B, SNAPS = ovn.N, ovn.T, ovn.STEPS, ovn.B, ovn.SNAPS
CONFIGS, F = ovn.GOLDEN_CONFIGS, ovn.F_GOLD


def compact_unrolling(snap):
    """(observations, terminals, row of every flat index) of the compact
    unrolling: each episode's rows followed by one extra row holding its last
    next_observations."""
    obs, term, umap = [], [], []
    for u in range(len(snap['terminals'])):
        umap.append(len(obs))
        obs.append(snap['observations'][u])
        term.append(0.0)
        if snap['terminals'][u] > 0:
            obs.append(snap['next_observations'][u])
            term.append(1.0)
    return np.array(obs), np.array(term, np.float32), np.array(umap, np.int64)


def episode_starts(done, S):
    """[N, L] for the live steps at S: (true start step of the row's episode,
    its first live step)."""
    L = min(S, T)
    true0 = np.zeros((N, L), np.int64)
    for e in range(N):
        for k in range(L):
            t = S - L + k
            s = t
            while s > 0 and not done[s - 1, e]:
                s -= 1
            true0[e, k] = s
    return true0, np.maximum(true0, S - L)


def stack_cases(done, S, rows, goal_rows):
    """The designed cases among the stacks of the flat rows ``rows`` (every
    selector's) and ``goal_rows`` (goals that differ from their sample)."""
    L = min(S, T)
    true0, live0 = episode_starts(done, S)
    c = dict(clamp_episode_start=0, clamp_oldest_live=0, crosses_wrap=0, length_one=0, goal_clamps=0)

    def one(u):
        e, k = divmod(int(u), L)
        t = S - L + k
        short = t - live0[e, k] < F - 1
        return e, t, short, true0[e, k], live0[e, k]

    for u in rows:
        e, t, short, t0, l0 = one(u)
        c['clamp_episode_start'] += int(short and l0 == t0)
        c['clamp_oldest_live'] += int(short and l0 > t0)
        steps = [max(t - i, l0) for i in reversed(range(F))]
        c['crosses_wrap'] += int(any(a % T == T - 1 and b == a + 1 for a, b in zip(steps, steps[1:])))
        c['length_one'] += int(t0 == t and done[t, e])
    for u in goal_rows:
        c['goal_clamps'] += int(one(u)[2])
    return c


def hgc_indices(h, idxs):
    """Key -> flat rows of HGCDataset.sample (datasets.py:496-619), by the
    reference's own calls in its order."""
    c = h.config
    fin = h.terminal_locs[np.searchsorted(h.terminal_locs, idxs)]
    hvg = h.sample_goals(idxs, c['value_p_curgoal'], c['value_p_trajgoal'], c['value_p_randomgoal'],
                         c['value_geom_sample'])
    high = c.get('high_subgoal_steps', c['subgoal_steps'])
    vsteps = high if c.get('value_subgoal_steps') is None else c['value_subgoal_steps']
    lsteps = c.get('low_subgoal_steps', c['subgoal_steps'])
    asteps = high if c.get('actor_subgoal_steps') is None else c['actor_subgoal_steps']
    hv_next, _ = h.compute_high_next_idxs(idxs, fin, hvg, vsteps)
    lv_next, _ = h.compute_high_next_idxs(idxs, fin, hvg, lsteps)
    lvg = h.sample_goals(idxs, c['value_p_curgoal'], c['value_p_trajgoal'], c['value_p_randomgoal'], geom_sample=True,
                         discount=c['low_discount'])
    hag = h.sample_goals(idxs, c['actor_p_curgoal'], c['actor_p_trajgoal'], c['actor_p_randomgoal'],
                         c['actor_geom_sample'])
    ha_next, _ = h.compute_high_next_idxs(idxs, fin, hag, asteps)
    la_goal = np.minimum(idxs + asteps, fin)
    la_next, _ = h.compute_high_next_idxs(idxs, fin, hag, lsteps)
    return dict(observations=idxs, high_value_reps=idxs, high_value_goals=hvg, value_goals=hvg,
                high_value_actions=hv_next, high_value_next_observations=hv_next,
                low_value_next_observations=lv_next, low_value_goals=lvg, high_actor_goals=hag,
                high_actor_actions=ha_next, high_actor_targets=ha_next, high_actor_next_observations=ha_next,
                low_actor_goals=la_goal, low_actor_goal_observations=la_goal, low_actor_next_observations=la_next)


def gc_indices(g, idxs):
    c = g.config
    vg = g.sample_goals(idxs, c['value_p_curgoal'], c['value_p_trajgoal'], c['value_p_randomgoal'],
                        c['value_geom_sample'])
    ag = g.sample_goals(idxs, c['actor_p_curgoal'], c['actor_p_trajgoal'], c['actor_p_randomgoal'],
                        c['actor_geom_sample'])
    return dict(observations=idxs, value_goals=vg, actor_goals=ag)


def one_batch(dsm, snap, cfg, hgc, seed):
    """(batch, draws with crop_from, key -> flat rows)."""
    cls = dsm.HGCDataset if hgc else dsm.GCDataset
    regular = {k: v.copy() for k, v in snap.items()}
    compact = {k: v.copy() for k, v in snap.items() if k != 'next_observations'}
    obs_u, term_u, umap = compact_unrolling(snap)
    no_stack = dict(cfg, frame_stack=None)
    plain = cls(dsm.Dataset.create(**regular), no_stack)
    stacker = cls(dsm.Dataset.create(**compact), dict(cfg), preprocess_frame_stack=False)
    unrolled = cls(dsm.Dataset.create(observations=obs_u, terminals=term_u), dict(cfg), preprocess_frame_stack=False)

    # the indices, by the reference's own calls in sample()'s order
    np.random.seed(seed)
    idxs = plain.dataset.get_random_idxs(B)
    index = (hgc_indices if hgc else gc_indices)(plain, idxs)

    real_augment = plain.augment

    def stack_then_augment(batch, keys):
        for key, rows in index.items():
            assert np.array_equal(batch[key], snap['observations'][rows]), key  # the key's index
        stacks = {}
        for key, rows in index.items():
            k = rows.tobytes()
            if k not in stacks:
                stacks[k] = stacker.get_stacked_observations(rows)
            batch[key] = stacks[k]  # high_value_reps is observations, as sample() binds it
        batch['next_observations'] = unrolled.get_stacked_observations(umap[idxs] + 1)
        real_augment(batch, keys)

    plain.augment = stack_then_augment
    np.random.seed(seed)
    with gg.Recorder() as rec:
        batch = plain.sample(B)
    log = rec.log  # the coin and augment()'s randint close the log
    assert log[-2][0] == 'rand' and log[-2][1].shape == () and log[-1][0] == 'randint'
    crop_from = log[-1][1].astype(np.int64)
    draws = (gg.hgc_draws_from_log if hgc else gg._draws_from_log)(log[:-2], B, cfg)
    draws.pop('l_dist', None)  # the low goal is always geometric: ogbx_hgc_draws has no such field
    assert np.array_equal(draws['pick'], idxs)
    draws['crop_from'] = crop_from
    return batch, draws, index


def main():
    _, dsm, _ = gg.reference_modules()
    gv.numpy_jax()
    rows, done = ovn.history()
    for t in range(STEPS - 1):  # the history's own premise
        same = ~done[t]
        assert np.array_equal(rows['next_observations'][t][same], rows['observations'][t + 1][same])
    out = {f'in_{k}': v for k, v in rows.items()}
    out['done'] = done
    out['snap_steps'] = np.array(SNAPS)
    dtypes = {k: v.dtype for k, v in rows.items()}
    model = onp.Brute(N, T)
    counts = dict(clamp_episode_start=0, clamp_oldest_live=0, crosses_wrap=0, length_one=0, goal_clamps=0)
    crops = np.zeros((2, 7), np.int64)
    for t in range(STEPS):
        model.add({k: v[t] for k, v in rows.items()}, done[t])
        S = t + 1
        if S not in SNAPS:
            continue
        snap = model.snapshot(dtypes)
        for cname, cfg in CONFIGS.items():
            hgc = ovn.HGC[cname]
            batch, draws, index = one_batch(dsm, snap, cfg, hgc, 1000 * S + sum(map(ord, cname)))
            for k, v in draws.items():
                out[f's{S}_{cname}_draw_{k}'] = v
            for k, v in batch.items():
                out[f's{S}_{cname}_out_{k}'] = np.asarray(v)
            out[f's{S}_{cname}_keys'] = np.array(list(batch.keys()))
            goal = index['high_value_goals' if hgc else 'value_goals']
            c = stack_cases(done, S, np.concatenate(list(index.values())), goal[goal != index['observations']])
            for k, v in c.items():
                counts[k] += v
            for ax in range(2):
                crops[ax] += np.bincount(draws['crop_from'][:, ax], minlength=7)
    assert all(v >= 1 for v in counts.values()), counts
    assert (crops[:, [0, 6]] >= 1).all(), crops
    path = os.path.join(HERE, 'online_visual_golden.npz')
    np.savez_compressed(path, **out)
    print('online visual golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes;', counts)
    print('  crop offsets per axis:', crops.tolist())
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, 'visual_golden.npz'))


if __name__ == '__main__':
    main()
