"""Golden fixtures for ATC batches (anchor / positive observation pairs), from
the reference's own ATCDataset (impls/utils/datasets.py:369-464).

Reuses make_golden_gc's loader of the reference modules and make_golden_visual's
NumPy stand-ins for the jax calls of the crop and its dataset builders.  Saves
arrays only (tests/golden/atc_golden.npz): per case the dataset
(``<case>_in_*``), ``<case>_k``, the reference's valid(k) (``<case>_valid``),
the rows np.random.choice drew (``<case>_idxs``) and their positions in
valid(k) (``<case>_draw_pick``), the coin and augment()'s offsets when the call
drew them (``<case>_draw_coin``, ``<case>_draw_crop_from``), the batch
(``<case>_out_*``) and its key order (``<case>_keys``).

Cases (batch 64, trajectory lengths make_golden_visual.LENGTHS)
  state        float32 observations (5,), no stack, p_aug None, k = 1
  stack_state  the same observations, frame_stack 3 per call, p_aug 1.0, k = 3:
               the coin and the offsets are drawn, nothing is cropped
  vis          uint8 frames 6 x 5 x 2, frame_stack 3 per call, p_aug 1.0, the
               default padding 4, k = 2: offsets up to 8 exceed both image sides
  vis_pre      vis with preprocess_frame_stack=True at the same NumPy seed
               (asserted equal to vis)
  vis_pad1     uint8 frames 7 x 5 x 3, augment_padding 1, no stack, p_aug 1.0,
               k = 7
  regular      non-compact uint8 4-D dataset without 'valids', p_aug 1.0, k = 4
  k_last       vis's dataset, frame_stack 3, k = 29: valid(k) is the first row
               of the 30-row trajectory
and the reference raises its ValueError at k = 30.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_gc as gg  # noqa: E402
import make_golden_visual as gv  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
B = 64


class Recorder:
    """Wrap np.random.{choice,rand,randint} and log (name, value) in order."""

    def __init__(self, names=('choice', 'rand', 'randint')):
        self.names, self.log, self._saved = names, [], {}

    def __enter__(self):
        for name in self.names:
            fn = getattr(np.random, name)
            self._saved[name] = fn

            def wrap(*a, _fn=fn, _name=name, **k):
                v = _fn(*a, **k)
                self.log.append((_name, np.array(v)))
                return v

            setattr(np.random, name, wrap)
        return self

    def __exit__(self, *exc):
        for k, fn in self._saved.items():
            setattr(np.random, k, fn)


def record(out, case, data, sampler, k, augments):
    for key, v in data.items():
        out[f'{case}_in_{key}'] = v
    with Recorder() as rec:
        batch = sampler.sample(B, k)
    log = rec.log
    valid = np.asarray(sampler.get_valid_atc_idxs(k), np.int64)
    assert log[0][0] == 'choice' and log[0][1].shape == (B,)
    idxs = log[0][1].astype(np.int64)
    pick = np.searchsorted(valid, idxs)
    assert np.array_equal(valid[pick], idxs)
    out[f'{case}_k'] = np.int64(k)
    out[f'{case}_valid'] = valid
    out[f'{case}_idxs'] = idxs
    out[f'{case}_draw_pick'] = pick.astype(np.int64)
    if augments:  # the coin and augment()'s randint close the log
        assert [n for n, _ in log] == ['choice', 'rand', 'randint'] and log[1][1].shape == ()
        out[f'{case}_draw_coin'] = log[1][1]
        out[f'{case}_draw_crop_from'] = log[2][1].astype(np.int64)
    else:
        assert [n for n, _ in log] == ['choice']
    for key, v in batch.items():
        out[f'{case}_out_{key}'] = np.asarray(v)
    out[f'{case}_keys'] = np.array(list(batch.keys()))
    return batch


def main():
    _, dsm, _ = gg.reference_modules()
    gv.numpy_jax()
    rng = np.random.RandomState(20250)
    out = {}

    def sampler(data, cfg, pre=False):
        return dsm.ATCDataset(dsm.Dataset.create(**data), dict(cfg), preprocess_frame_stack=pre)

    data_s = gv.compact_dataset(rng, (5,), np.float32)
    np.random.seed(201)
    record(out, 'state', data_s, sampler(data_s, dict(frame_stack=None, p_aug=None)), 1, False)
    np.random.seed(202)
    record(out, 'stack_state', data_s, sampler(data_s, dict(frame_stack=3, p_aug=1.0)), 3, True)

    data_v = gv.compact_dataset(rng, (6, 5, 2), np.uint8)
    cfg_v = dict(frame_stack=3, p_aug=1.0)
    np.random.seed(203)
    vis = record(out, 'vis', data_v, sampler(data_v, cfg_v), 2, True)
    np.random.seed(203)  # the reference's two stacking modes agree
    pre = record(out, 'vis_pre', data_v, sampler(data_v, cfg_v, pre=True), 2, True)
    assert list(vis) == list(pre) and all(np.array_equal(vis[key], pre[key]) for key in vis)
    assert out['vis_draw_crop_from'].max() == 8 and out['vis_draw_crop_from'].min() == 0

    data_p = gv.compact_dataset(rng, (7, 5, 3), np.uint8)
    np.random.seed(204)
    record(out, 'vis_pad1', data_p, sampler(data_p, dict(frame_stack=None, p_aug=1.0, augment_padding=1)), 7, True)

    data_r = gv.regular_dataset(rng, (6, 5, 2))
    assert 'valids' not in data_r
    np.random.seed(205)
    record(out, 'regular', data_r, sampler(data_r, dict(frame_stack=None, p_aug=1.0)), 4, True)

    last = sampler(data_v, dict(frame_stack=3, p_aug=None))
    np.random.seed(206)
    record(out, 'k_last', data_v, last, 29, False)
    first = int(np.cumsum(gv.LENGTHS)[5])  # first row of the 30-row trajectory
    assert out['k_last_valid'].tolist() == [first]
    try:
        last.sample(B, 30)
    except ValueError as e:
        assert str(e) == 'No valid ATC indices found for k=30.'
    else:
        raise AssertionError('the reference accepted k = 30')

    path = os.path.join(OUT, 'atc_golden.npz')
    np.savez_compressed(path, **out)
    print('atc golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
