"""Golden fixtures for TRL batches over the episode ring
(include/ogbx_online_trl.h, a ``GCReplayBuffer`` whose config has a TRL agent
name), from the reference's own ``GCDataset`` with ``agent_name='trl'``
(impls/utils/datasets.py:198-204, 254-276).

Reuses make_golden_online's scripted history (N = 5 envs, T = 6 slots, 17
steps, kept as plain per-env lists by tests/online_np.Brute: no ring, no
table) and make_golden_trl's recorder of one sample call.  At steps 2, 3, 6, 11
and 17 the live rows are laid out as a dataset and the reference's
``GCDataset.sample(64)`` runs over it for trl_np.STATE_CFG (geometric value
goals) and its ``value_geom_sample=False`` variant.  Saves arrays only
(tests/golden/online_trl_golden.npz):

  hist_<key> [17, 5, ...], done [17, 5], snap_steps   the history
  s<S>_<cfg>_in_<key>                      the snapshot dataset at step S
  s<S>_<cfg>_draw_<name>                   the eleven GC draws and ``midpoint``
  s<S>_<cfg>_log<i>_<fn>                   every np.random draw in call order
  s<S>_<cfg>_out_<key>, s<S>_<cfg>_keys    the batch and its key order
  s<S>_pickable                            the size of the reference's pick table

``counts`` are asserted >= 1 each, from the model alone (the done pattern, the
recorded draws and tests/trl_np.py over the snapshot): a sample of span 1, one
of a longer span whose midpoint lies strictly inside, a sample in an episode
whose head was overwritten, a sample in the open episode that wraps the ring,
an actor random goal in another env.  S = 2 has an env without a pickable row.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_gc as gg  # noqa: E402
import make_golden_online as go  # noqa: E402
import make_golden_trl as gt  # noqa: E402
import online_np as onp  # noqa: E402
import online_trl_np as otn  # noqa: E402
import trl_np as tnp  # noqa: E402

N, T, STEPS, B = go.N, go.T, go.STEPS, gt.B
SNAPS = (2, 3, 6, 11, 17)
CONFIGS = otn.CONFIGS


def sample_counts(done, S, cfg, draws, ix):
    """The designed cases among one call's samples."""
    L = min(S, T)
    t0 = S - L
    e, k = ix['idxs'] // L, ix['idxs'] % L
    step = t0 + k
    c = dict(span_one=0, mid_inside=0, head_overwritten=0, open_wraps=0, random_other_env=0)
    span = ix['vg'] - ix['idxs']
    c['span_one'] = int((span == 1).sum())
    c['mid_inside'] = int(((span > 1) & (ix['idxs'] < ix['mid']) & (ix['mid'] < ix['vg'])).sum())
    for b in range(len(e)):
        ends = np.flatnonzero(done[:S, e[b]])
        before = ends[ends < step[b]]
        start = int(before[-1]) + 1 if len(before) else 0
        c['head_overwritten'] += int(start < t0)
        is_open = not (ends >= step[b]).any()
        c['open_wraps'] += int(is_open and any(t % T == T - 1 for t in range(max(start, t0), S - 1)))
    thresh = cfg['actor_p_trajgoal'] / (1.0 - cfg['actor_p_curgoal'])
    is_rand = ~(draws['a_u_cur'] < cfg['actor_p_curgoal']) & ~(draws['a_u_traj'] < thresh)
    c['random_other_env'] = int((is_rand & (ix['ag'] // L != e)).sum())
    return c


def main():
    _, dsm, _ = gg.reference_modules()
    rows, done = go.history()
    out = {f'hist_{k}': v for k, v in rows.items()}
    out['done'] = done
    out['snap_steps'] = np.array(SNAPS)
    dtypes = {k: v.dtype for k, v in rows.items()}
    model = onp.Brute(N, T)
    total = {}
    for t in range(STEPS):
        model.add({k: v[t] for k, v in rows.items()}, done[t])
        S = t + 1
        if S not in SNAPS:
            continue
        snap = model.snapshot(dtypes)
        table = tnp.pick_table(snap['terminals'])
        out[f's{S}_pickable'] = np.array(len(table))
        envs_hit = set()
        for cname, cfg in CONFIGS.items():
            case = f's{S}_{cname}'
            gc = dsm.GCDataset(dsm.Dataset.create(**{k: v.copy() for k, v in snap.items()}), dict(cfg))
            assert np.array_equal(gc.dataset.valid_idxs, table)
            np.random.seed(1000 * S + sum(map(ord, cname)))
            batch = gt.record(out, case, snap, gc, cfg)
            draws = {k[len(case) + 6:]: v for k, v in out.items() if k.startswith(case + '_draw_')}
            exp, ix = tnp.batch(snap, cfg, draws)
            assert list(exp) == list(batch), (case, list(exp), list(batch))
            for k, v in batch.items():
                v = np.asarray(v)
                assert exp[k].dtype == v.dtype and np.array_equal(exp[k], v), (case, k)
            for k, v in sample_counts(done, S, cfg, draws, ix).items():
                total[k] = total.get(k, 0) + v
            envs_hit |= set((ix['idxs'] // min(S, T)).tolist())
        pickable = {int(u) // min(S, T) for u in table}
        assert envs_hit == pickable, (S, envs_hit, pickable)
        assert (len(pickable) < N) == (S == 2), (S, pickable)
    assert all(v >= 1 for v in total.values()), total
    path = os.path.join(HERE, 'online_trl_golden.npz')
    np.savez_compressed(path, **out)
    print('online trl golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes;', total,
          {S: int(out[f's{S}_pickable']) for S in SNAPS})


if __name__ == '__main__':
    main()
