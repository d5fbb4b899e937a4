"""Golden fixtures for hierarchical hindsight sampling over the episode ring
(include/ogbx_online_hgc.h, ``HGCReplayBuffer``), from the reference's own
``HGCDataset`` (impls/utils/datasets.py:467-643).

Reuses make_golden_gc's loader of the reference modules, its recorder of
np.random draws and ``hgc_draws_from_log``.  The history of make_golden_online
is too short for subgoals (T = 6: every subgoal step is clipped by the episode
end), so this one has N = 5 envs, T = 12 slots and 31 steps, kept as plain
per-env lists (tests/online_np.Brute: no ring, no table); at steps 4, 12, 20
and 31 the live rows are laid out as a dataset and the reference's
``HGCDataset.sample(64)`` runs over it for three configs
(tests/online_hgc_np.GOLDEN_CONFIGS: make_golden_gc.HGC_CONFIGS with the steps
shortened to the ring).  Saves arrays only
(tests/golden/online_hgc_golden.npz):

  in_<key> [31, 5, ...], done [31, 5]       the history
  s<S>_snap_<key>                           the snapshot dataset at step S
  s<S>_<cfg>_draw_<name>, s<S>_<cfg>_out_<key>, s<S>_<cfg>_keys
                                            the recorded draws (names as
                                            ogbx_hgc_draws), the batch and its
                                            key order

Asserted >= 1 each: the done-pattern counts of make_golden_online (but
``same_step``: no two envs of this scripted pattern are done on one step;
online_golden.npz and the random histories of the GPU tests hold that case)
and, for ``hiql`` and ``hlow`` summed over the snapshots, the regimes of
``high_value_subgoal_steps`` (online_hgc_np.REGIMES).
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
import online_hgc_np as ohn  # noqa: E402
import online_np as onp  # noqa: E402
from oracle import gcdataset_np as gco  # noqa: E402

N, T, STEPS, B, SNAPS, DONE_AT = ohn.N, ohn.T, ohn.STEPS, ohn.B, ohn.SNAPS, ohn.DONE_AT
CONFIGS = ohn.GOLDEN_CONFIGS
EXAMPLE = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))


def history():
    """Rows drawn like make_golden_online.history()."""
    rng = np.random.RandomState(20)
    done = np.zeros((STEPS, N), bool)
    for e, steps in DONE_AT.items():
        done[list(steps), e] = True
    rows = dict(observations=rng.randint(-99, 100, (STEPS, N, 2)).astype(np.float64),
                actions=rng.randint(-9, 10, (STEPS, N, 2)).astype(np.float32),
                next_observations=rng.randint(-99, 100, (STEPS, N, 2)).astype(np.float64))
    return rows, done


def pattern_counts(done):
    """make_golden_online.pattern_counts over this history's shape."""
    saved = go.N, go.T, go.SNAPS
    go.N, go.T, go.SNAPS = N, T, SNAPS
    try:
        return go.pattern_counts(done)
    finally:
        go.N, go.T, go.SNAPS = saved


def main():
    _, dsm, _ = gg.reference_modules()
    for name, cfg in CONFIGS.items():  # derived from the reference-pinned configs, only the steps differ
        steps = ('subgoal_steps', 'high_subgoal_steps', 'value_subgoal_steps', 'actor_subgoal_steps',
                 'low_subgoal_steps')
        assert {k: v for k, v in cfg.items() if k not in steps} == \
            {k: v for k, v in gg.HGC_CONFIGS[name].items() if k not in steps}, name
    rows, done = history()
    counts = pattern_counts(done)
    assert all(v >= 1 for k, v in counts.items() if k != 'same_step') and counts['same_step'] == 0, counts
    out = {f'in_{k}': v for k, v in rows.items()}
    out['done'] = done
    out['snap_steps'] = np.array(SNAPS)
    dtypes = {k: v.dtype for k, v in rows.items()}
    model, ring = onp.Brute(N, T), onp.OnlineNp(EXAMPLE, N, T)
    seen = {c: dict.fromkeys(ohn.REGIMES, 0) for c in CONFIGS}
    nkeys = {}
    for t in range(STEPS):
        model.add({k: v[t] for k, v in rows.items()}, done[t])
        ring.add({k: v[t] for k, v in rows.items()}, done[t])
        S = t + 1
        if S not in SNAPS:
            continue
        snap = model.snapshot(dtypes)
        for k, v in snap.items():
            out[f's{S}_snap_{k}'] = v
        for cname, cfg in CONFIGS.items():
            hgc = dsm.HGCDataset(dsm.Dataset.create(**{k: v.copy() for k, v in snap.items()}), dict(cfg))
            np.random.seed(1000 * S + sum(map(ord, cname)))
            with gg.Recorder() as rec:
                batch = hgc.sample(B)
            draws = gg.hgc_draws_from_log(rec.log, B, cfg)
            draws.pop('l_dist', None)  # the low goal is always geometric: ogbx_hgc_draws has no such field
            for k, v in draws.items():
                out[f's{S}_{cname}_draw_{k}'] = v
            for k, v in batch.items():
                out[f's{S}_{cname}_out_{k}'] = np.asarray(v)
            out[f's{S}_{cname}_keys'] = np.array(list(batch.keys()))
            nkeys[cname] = len(batch)
            # the restatement equals the reference bit for bit
            exp, ix = gco.hgc_sample(snap, cfg, draws)
            assert list(exp) == list(batch.keys()), (S, cname)
            for k, v in batch.items():
                v = np.asarray(v)
                assert exp[k].dtype == v.dtype and exp[k].shape == v.shape and np.array_equal(exp[k], v), (S, cname, k)
            r = ohn.regimes(ring, ix['idxs'], ix['hvg'], exp['high_value_subgoal_steps'], ohn.value_steps(cfg))
            for k, v in r.items():
                seen[cname][k] += v
    assert nkeys == dict(hiql=26, hlow=27, hcur=27), nkeys
    for cname in ('hiql', 'hlow'):
        assert all(v >= 1 for v in seen[cname].values()), (cname, seen[cname])
    np.savez_compressed(os.path.join(HERE, 'online_hgc_golden.npz'), **out)
    print('online hgc golden:', len(out), 'arrays;', counts)
    for cname, r in seen.items():
        print(' ', cname, r)


if __name__ == '__main__':
    main()
