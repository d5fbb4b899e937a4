"""Golden fixtures for visual batches (frame stack and random crop), from the
reference's own GCDataset / HGCDataset (impls/utils/datasets.py).

Reuses make_golden_gc's loader of the reference modules and its np.random
recorder, and gives the jax stand-ins the three functions the crop needs as
NumPy code written here: ``jnp.pad`` (np.pad), ``jax.lax.dynamic_slice``
(slicing) and ``jax.vmap`` (a loop).  Saves arrays only
(tests/golden/visual_golden.npz): per case the dataset (``<case>_in_*``), the
named draws of the sample call (``<case>_draw_*``, with ``coin`` and
``crop_from`` when the call augmented), every np.random draw in call order
(``<case>_log<i>_<fn>``) and the batch (``<case>_out_*``).

Cases
  A  GC, uint8 frames 6 x 5 x 2 (H != W, 10-byte rows), trajectories of 2 and 3
     rows (< F) and long ones, frame_stack 3, p_aug 1.0, batch 64, stacking per
     call (preprocess_frame_stack=False; asserted equal to True)
  B  as A with uint8 8 x 8 x 4 frames (16-byte aligned rows), preprocessed stack
  C  float32 2-D observations, frame_stack 3
  D  case A under evaluation=True
  E  HGC on A's dataset with low_discount
  F  crop only (frame_stack None) on a non-compact dataset
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_gc as gg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

GC_CFG = dict(gg.CONFIGS['gciql'], frame_stack=3, p_aug=1.0)
HGC_CFG = dict(gg.HGC_CONFIGS['hlow'], frame_stack=3, p_aug=1.0)
LENGTHS = [2, 3, 17, 3, 2, 9, 30, 4, 2, 25]
B = 64


def numpy_jax():
    """Working NumPy stand-ins for the jax calls of random_crop / batched_random_crop."""
    jax = sys.modules['jax']
    jax.numpy.pad = np.pad

    def dynamic_slice(operand, start_indices, slice_sizes):
        # lax.dynamic_slice moves an out-of-range start into range
        start = [int(np.clip(s, 0, d - n)) for s, d, n in zip(start_indices, operand.shape, slice_sizes)]
        return operand[tuple(slice(s, s + n) for s, n in zip(start, slice_sizes))]

    def vmap(f, in_axes=0):
        def batched(*args):
            n = len(next(a for a, ax in zip(args, in_axes) if ax is not None))
            return np.stack([f(*[a[i] if ax is not None else a for a, ax in zip(args, in_axes)]) for i in range(n)])
        return batched

    jax.lax.dynamic_slice = dynamic_slice
    jax.vmap = vmap


def compact_dataset(rng, frame_shape, dtype, lengths=LENGTHS):
    """A compact (observation-only) dataset as load_dataset(compact_dataset=True)
    lays it out: terminals at each trajectory's last row, valids = 1 - terminals."""
    R = sum(lengths)
    if dtype == np.uint8:
        obs = rng.randint(0, 256, (R,) + frame_shape).astype(np.uint8)
    else:
        obs = rng.normal(size=(R,) + frame_shape).astype(dtype)
    term = np.zeros(R, np.float32)
    term[np.cumsum(lengths) - 1] = 1
    return dict(observations=obs, actions=rng.uniform(-1, 1, (R, 2)).astype(np.float32), terminals=term,
                valids=1.0 - term)


def regular_dataset(rng, frame_shape, lengths=LENGTHS):
    """A non-compact dataset (load_dataset(compact_dataset=False)): the last
    row of each trajectory dropped, next_observations stored."""
    full = compact_dataset(rng, frame_shape, np.uint8, [n + 1 for n in lengths])
    keep = full['terminals'] == 0
    nxt = np.roll(keep, 1)
    nxt[0] = False
    term = np.zeros(int(keep.sum()), np.float32)
    term[np.cumsum(lengths) - 1] = 1
    return dict(observations=full['observations'][keep], next_observations=full['observations'][nxt],
                actions=full['actions'][keep], terminals=term)


def record(out, case, data, sampler, cfg, hgc, evaluation=False):
    for k, v in data.items():
        out[f'{case}_in_{k}'] = v
    with gg.Recorder() as rec:
        batch = sampler.sample(B, evaluation=evaluation)
    log = rec.log
    for i, (name, v) in enumerate(log):
        out[f'{case}_log{i:02d}_{name}'] = v
    if not evaluation:  # the coin and augment()'s randint close the log
        assert log[-2][0] == 'rand' and log[-2][1].shape == () and log[-1][0] == 'randint'
        out[f'{case}_draw_coin'] = log[-2][1]
        out[f'{case}_draw_crop_from'] = log[-1][1].astype(np.int64)
        log = log[:-2]
    draws = gg.hgc_draws_from_log(log, B, cfg) if hgc else gg._draws_from_log(log, B, cfg)
    for k, v in draws.items():
        out[f'{case}_draw_{k}'] = v
    for k, v in batch.items():
        out[f'{case}_out_{k}'] = np.asarray(v)
    return batch


def main():
    _, dsm, _ = gg.reference_modules()
    numpy_jax()
    rng = np.random.RandomState(20240)
    out = {}

    data_a = compact_dataset(rng, (6, 5, 2), np.uint8)
    np.random.seed(101)
    batch = record(out, 'A', data_a, dsm.GCDataset(dsm.Dataset.create(**data_a), dict(GC_CFG),
                                                  preprocess_frame_stack=False), GC_CFG, False)
    np.random.seed(101)  # the reference's two stacking modes agree
    other = dsm.GCDataset(dsm.Dataset.create(**data_a), dict(GC_CFG), preprocess_frame_stack=True).sample(B)
    assert all(np.array_equal(batch[k], other[k]) for k in ('observations', 'next_observations', 'value_goals',
                                                            'actor_goals'))

    data_b = compact_dataset(rng, (8, 8, 4), np.uint8)
    np.random.seed(102)
    record(out, 'B', data_b, dsm.GCDataset(dsm.Dataset.create(**data_b), dict(GC_CFG),
                                          preprocess_frame_stack=True), GC_CFG, False)

    data_c = compact_dataset(rng, (5,), np.float32)
    np.random.seed(103)
    record(out, 'C', data_c, dsm.GCDataset(dsm.Dataset.create(**data_c), dict(GC_CFG),
                                          preprocess_frame_stack=False), GC_CFG, False)

    np.random.seed(104)
    record(out, 'D', data_a, dsm.GCDataset(dsm.Dataset.create(**data_a), dict(GC_CFG),
                                          preprocess_frame_stack=False), GC_CFG, False, evaluation=True)

    np.random.seed(105)
    record(out, 'E', data_a, dsm.HGCDataset(dsm.Dataset.create(**data_a), dict(HGC_CFG),
                                           preprocess_frame_stack=False), HGC_CFG, True)

    data_f = regular_dataset(rng, (6, 5, 2))
    cfg_f = dict(GC_CFG, frame_stack=None)
    np.random.seed(106)
    record(out, 'F', data_f, dsm.GCDataset(dsm.Dataset.create(**data_f), dict(cfg_f)), cfg_f, False)

    path = os.path.join(OUT, 'visual_golden.npz')
    np.savez_compressed(path, **out)
    print('visual golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
