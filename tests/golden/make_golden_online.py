"""Golden fixtures for hindsight sampling over the episode ring
(include/ogbx_online.h, ``GCReplayBuffer``), from the reference's own
``GCDataset`` (impls/utils/datasets.py:149-327).

Reuses make_golden_gc's loader of the reference modules and its recorder of
np.random draws.  A scripted history of N = 5 envs, T = 6 slots and 17 steps is
kept as plain per-env lists (tests/online_np.Brute: no ring, no table); at
steps 3, 6, 11 and 17 the live rows are laid out as a dataset (env-major,
terminals on the last row of every closed episode and on every env's newest
row) and the reference's ``GCDataset.sample(64)`` runs over it for four
configs: geometric / uniform trajectory goals x gc_negative on / off.  Saves
arrays only (tests/golden/online_golden.npz):

  in_<key> [17, 5, ...], done [17, 5]       the history
  s<S>_snap_<key>                           the snapshot dataset at step S
  s<S>_<cfg>_draw_<name>, s<S>_<cfg>_out_<key>   the recorded draws (names as
                                            ogbx_gc_draws) and the batch

The done pattern is designed; ``counts`` are asserted >= 1 each:
  an episode of length 1, two envs done on one step, an env that is never
  done, an episode whose head was overwritten at a snapshot, an open episode
  that wraps the ring at a snapshot.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_gc as gg  # noqa: E402
import online_np as onp  # noqa: E402

N, T, STEPS, B = 5, 6, 17, 64
SNAPS = (3, 6, 11, 17)
DONE_AT = {0: (2, 3, 9, 14), 1: (3, 10), 2: (0, 7, 8, 15), 3: (6, 12), 4: ()}
CONFIGS = onp.GOLDEN_CONFIGS


def history():
    rng = np.random.RandomState(20)
    done = np.zeros((STEPS, N), bool)
    for e, steps in DONE_AT.items():
        done[list(steps), e] = True
    rows = dict(observations=rng.randint(-99, 100, (STEPS, N, 2)).astype(np.float64),
                actions=rng.randint(-9, 10, (STEPS, N, 2)).astype(np.float32),
                next_observations=rng.randint(-99, 100, (STEPS, N, 2)).astype(np.float64))
    return rows, done


def pattern_counts(done):
    """The designed cases, counted from the done pattern alone."""
    c = dict(length_one=0, same_step=0, never_done=0, head_overwritten=0, open_wraps=0)
    c['same_step'] = int((done.sum(1) >= 2).sum())
    c['never_done'] = int((~done.any(0)).sum())
    for e in range(N):
        ends = np.flatnonzero(done[:, e])
        starts = np.concatenate([[0], ends + 1])
        c['length_one'] += int(sum(1 for s, t in zip(starts, ends) if s == t))
        for S in SNAPS:
            first = S - min(S, T)
            # the episode of the oldest live row started before it
            start = starts[np.searchsorted(ends, first)] if len(ends) else 0
            c['head_overwritten'] += int(start < first)
            # the open episode at S holds rows on both sides of slot T - 1 -> 0
            open_start = max(int(ends[ends < S][-1]) + 1 if (ends < S).any() else 0, first)
            c['open_wraps'] += int(any(t % T == T - 1 for t in range(open_start, S - 1)))
    return c


def main():
    _, dsm, _ = gg.reference_modules()
    rows, done = history()
    counts = pattern_counts(done)
    assert all(v >= 1 for v in counts.values()), counts
    out = {f'in_{k}': v for k, v in rows.items()}
    out['done'] = done
    out['snap_steps'] = np.array(SNAPS)
    dtypes = {k: v.dtype for k, v in rows.items()}
    model = onp.Brute(N, T)
    for t in range(STEPS):
        model.add({k: v[t] for k, v in rows.items()}, done[t])
        S = t + 1
        if S not in SNAPS:
            continue
        snap = model.snapshot(dtypes)
        for k, v in snap.items():
            out[f's{S}_snap_{k}'] = v
        for cname, cfg in CONFIGS.items():
            gc = dsm.GCDataset(dsm.Dataset.create(**{k: v.copy() for k, v in snap.items()}), dict(cfg))
            np.random.seed(1000 * S + sum(map(ord, cname)))
            with gg.Recorder() as rec:
                batch = gc.sample(B)
            for k, v in gg._draws_from_log(rec.log, B, cfg).items():
                out[f's{S}_{cname}_draw_{k}'] = v
            for k, v in batch.items():
                out[f's{S}_{cname}_out_{k}'] = np.asarray(v)
            out[f's{S}_{cname}_keys'] = np.array(list(batch.keys()))
    np.savez_compressed(os.path.join(HERE, 'online_golden.npz'), **out)
    print('online golden:', len(out), 'arrays;', counts)


if __name__ == '__main__':
    main()
