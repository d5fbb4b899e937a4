"""Golden fixtures for ATC batches over the episode ring
(include/ogbx_online_atc.h, ``GCReplayBuffer.sample_atc``), from the
reference's own ``ATCDataset`` (impls/utils/datasets.py:369-464).

Reuses make_golden_gc's loader of the reference modules, make_golden_visual's
NumPy stand-ins for the jax calls of the crop and make_golden_atc's recorder of
np.random draws.  The history is make_golden_online's designed one -- N = 5
envs, T = 6 slots, 17 steps, its done pattern -- kept as plain per-env lists
(tests/online_np.Brute: no ring, no table), in two forms: the uint8 6 x 5 x 2
frames of tests/online_visual_np.history (``vis``: frame_stack 3, p_aug 1) and
make_golden_online's float64 state rows (``state``: frame_stack None, p_aug
None).  At steps 3, 6, 11 and 17 the live rows are laid out as the dataset
``{observations, terminals}`` (next_observations dropped, as the reference
requires for frame_stack) and the reference's ``ATCDataset.sample(64, k)`` runs
over it for k = 1, 2, 3.

Saves arrays only (tests/golden/online_atc_golden.npz):

  vis_in_observations, state_in_observations [17, 5, ...], done [17, 5],
  snap_steps, ks                                       the history
  s<S>_k<k>_valid                                      the reference's valid(k)
  s<S>_k<k>_<form>_idxs, _draw_pick, _draw_crop_from   the rows np.random.choice
                                                       drew, their positions in
                                                       valid(k), augment()'s
                                                       offsets (vis)
  s<S>_k<k>_<form>_out_<key>, _keys                    the batch, its key order
  s3_k3_error                                          the reference's message
                                                       for its empty valid(3)

``counts`` are asserted at the (S, k) the history was designed for: an env
with no anchor while others have some; a segment without an anchor between two
that have some; anchors in a segment whose head was overwritten; a pair whose
anchor and positive straddle the physical wrap from slot T - 1 to slot 0; an
empty valid(k).  The valid(k) sizes run from 0 to 22.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_atc as ga  # noqa: E402
import make_golden_gc as gg  # noqa: E402
import make_golden_online as go  # noqa: E402
import make_golden_visual as gv  # noqa: E402
import online_atc_np as oan  # noqa: E402
import online_np as onp  # noqa: E402
import online_visual_np as ovn  # noqa: E402

N, T, STEPS, B, SNAPS = ovn.N, ovn.T, ovn.STEPS, ovn.B, ovn.SNAPS
KS = (1, 2, 3)
FORMS = {'vis': dict(frame_stack=3, p_aug=1.0), 'state': dict(frame_stack=None, p_aug=None)}


def designed_cases(ring, done, k, valid):
    """The designed cases at one (S, k), from the done pattern and the
    restatement's segments."""
    S, L = ring.S, ring.L
    t0 = S - L
    c = dict(env_without=0, gap_segment=0, head_overwritten=0, straddles_wrap=0)
    per_env = []
    for e in range(N):
        _, _, segs = oan.segments(ring, e)
        w = [max(E - b + 1 - k, 0) for b, E in segs]
        per_env.append(sum(w))
        c['gap_segment'] += int(any(w[i] == 0 and any(w[:i]) and any(w[i + 1:]) for i in range(len(w))))
        c['head_overwritten'] += int(t0 > 0 and not done[t0 - 1, e] and w[0] > 0)
    c['env_without'] = int(min(per_env) == 0 and max(per_env) > 0)
    steps = t0 + valid % L
    c['straddles_wrap'] = int(((steps % T) > ((steps + k) % T)).sum()) if k < T else 0
    return c


def main():
    _, dsm, _ = gg.reference_modules()
    gv.numpy_jax()
    vis_rows, done = ovn.history()
    state_rows, done_s = go.history()
    assert np.array_equal(done, done_s)
    rows = dict(vis=vis_rows['observations'], state=state_rows['observations'])
    out = {f'{form}_in_observations': v for form, v in rows.items()}
    out['done'] = done
    out['snap_steps'] = np.array(SNAPS)
    out['ks'] = np.array(KS)
    models = {form: onp.Brute(N, T) for form in rows}
    ring = onp.OnlineNp(dict(observations=np.zeros(ovn.FRAME, np.uint8)), N, T)
    cases, sizes = {}, []
    for t in range(STEPS):
        for form, m in models.items():
            m.add(dict(observations=rows[form][t]), done[t])
        ring.add(dict(observations=rows['vis'][t]), done[t])
        S = t + 1
        if S not in SNAPS:
            continue
        for k in KS:
            valid = None
            for form, cfg in FORMS.items():
                snap = models[form].snapshot(dict(observations=rows[form].dtype))
                ds = dsm.ATCDataset(dsm.Dataset.create(**{key: v.copy() for key, v in snap.items()}), dict(cfg))
                try:
                    v = np.asarray(ds.get_valid_atc_idxs(k), np.int64)
                except ValueError:  # it raises on an empty table; sample() below repeats it
                    v = np.zeros(0, np.int64)
                assert valid is None or np.array_equal(valid, v)
                valid = v
                np.random.seed(1000 * S + 10 * k + len(form))
                tag = f's{S}_k{k}_{form}'
                if len(valid) == 0:
                    try:
                        ds.sample(B, k)
                    except ValueError as err:
                        assert str(err) == f'No valid ATC indices found for k={k}.'
                        out[f's{S}_k{k}_error'] = np.array(str(err))
                    else:
                        raise AssertionError('the reference sampled an empty valid(k)')
                    continue
                with ga.Recorder() as rec:
                    batch = ds.sample(B, k)
                log = rec.log
                assert log[0][0] == 'choice' and log[0][1].shape == (B,)
                idxs = log[0][1].astype(np.int64)
                pick = np.searchsorted(valid, idxs)
                assert np.array_equal(valid[pick], idxs)
                out[f'{tag}_idxs'] = idxs
                out[f'{tag}_draw_pick'] = pick.astype(np.int64)
                if cfg['p_aug'] is not None:  # the coin and augment()'s randint close the log
                    assert [n for n, _ in log] == ['choice', 'rand', 'randint'] and log[1][1].shape == ()
                    out[f'{tag}_draw_crop_from'] = log[2][1].astype(np.int64)
                else:
                    assert [n for n, _ in log] == ['choice']
                for key, val in batch.items():
                    out[f'{tag}_out_{key}'] = np.asarray(val)
                out[f'{tag}_keys'] = np.array(list(batch.keys()))
            out[f's{S}_k{k}_valid'] = valid
            # the picks in order are the closed form's
            assert np.array_equal(oan.pick_rows(ring, k), valid), (S, k)
            cases[S, k] = designed_cases(ring, done, k, valid)
            sizes.append(len(valid))
    for key in ((3, 2), (6, 3), (11, 3)):
        assert cases[key]['env_without'] >= 1, (key, cases[key])
    for key in ((6, 1), (11, 1)):
        assert cases[key]['gap_segment'] >= 1, (key, cases[key])
    for (S, k), c in cases.items():
        if S >= 11:
            assert c['head_overwritten'] >= 1 and c['straddles_wrap'] >= 1, (S, k, c)
    assert len(out['s3_k3_valid']) == 0 and 's3_k3_error' in out
    assert min(sizes) == 0 and max(sizes) == 22, sizes
    path = os.path.join(HERE, 'online_atc_golden.npz')
    np.savez_compressed(path, **out)
    print('online atc golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes; valid(k) sizes', sizes)
    for key, c in cases.items():
        print(' ', key, c)


if __name__ == '__main__':
    main()
