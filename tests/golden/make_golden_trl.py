"""Golden fixtures for TRL batches of GCDataset (the value midpoint and the
keys around it), from the reference's own GCDataset with a TRL agent name
(impls/utils/datasets.py:198-204, 254-292).

Reuses make_golden_gc's loader of the reference modules and its np.random
recorder, and make_golden_visual's NumPy stand-ins for the crop and its dataset
builders.  Saves arrays only (tests/golden/trl_golden.npz): per case the
dataset (``<case>_in_*``), the named draws of the sample call
(``<case>_draw_*``: the eleven GC draws, ``midpoint`` -- the raw result of
``randint(idxs, value_goal_idxs)`` -- and, when the call augmented, ``coin`` and
``crop_from``), every np.random draw in call order (``<case>_log<i>_<fn>``),
the batch (``<case>_out_*``) and its key order (``<case>_keys``).

All cases: batch 64, trajectory lengths [2, 3, 17, 3, 2, 9, 30, 4, 2, 25]
(length-2 trajectories force the span to 1; some are shorter than the stack).

  state    compact, float32 observations (5,) (20-byte rows), actions (2,);
           the crl sampling probabilities, agent_name 'trl', discount 0.9,
           geometric value goals
  reps     as state plus oracle_reps (2,); value_geom_sample False
  regular  non-compact (no 'valids': the TRL pick table differs from "every
           row"), config of state
  vis      uint8 frames 6 x 5 x 2, frame_stack 3, p_aug 1.0, stacking per call,
           agent_name 'latent_trl'
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_gc as gg  # noqa: E402
import make_golden_visual as gv  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
B = 64

STATE_CFG = dict(gg.CONFIGS['crl'], agent_name='trl', discount=0.9, value_geom_sample=True)
REPS_CFG = dict(STATE_CFG, value_geom_sample=False)
VIS_CFG = dict(STATE_CFG, agent_name='latent_trl', frame_stack=3, p_aug=1.0)


def record(out, case, data, sampler, cfg):
    for k, v in data.items():
        out[f'{case}_in_{k}'] = v
    with gg.Recorder() as rec:
        batch = sampler.sample(B)
    log = rec.log
    for i, (name, v) in enumerate(log):
        out[f'{case}_log{i:02d}_{name}'] = v
    # pick, value goals (4), actor goals (4), midpoint, [coin, [crop]]
    assert [n for n, _ in log[:10]] == ['randint', 'randint', 'geometric' if cfg['value_geom_sample'] else 'rand',
                                        'rand', 'rand', 'randint', 'rand', 'rand', 'rand', 'randint']
    for k, v in gg._draws_from_log(log[:9], B, cfg).items():
        out[f'{case}_draw_{k}'] = v
    out[f'{case}_draw_midpoint'] = log[9][1].astype(np.int64)
    if cfg['p_aug'] is not None:
        assert len(log) == 12 and log[10][0] == 'rand' and log[10][1].shape == () and log[11][0] == 'randint'
        out[f'{case}_draw_coin'] = log[10][1]
        out[f'{case}_draw_crop_from'] = log[11][1].astype(np.int64)
    else:
        assert len(log) == 10
    for k, v in batch.items():
        out[f'{case}_out_{k}'] = np.asarray(v)
    out[f'{case}_keys'] = np.array(list(batch.keys()))
    return batch


def main():
    _, dsm, _ = gg.reference_modules()
    gv.numpy_jax()
    rng = np.random.RandomState(31337)
    out = {}

    data = gv.compact_dataset(rng, (5,), np.float32)
    np.random.seed(201)
    record(out, 'state', data, dsm.GCDataset(dsm.Dataset.create(**data), dict(STATE_CFG)), STATE_CFG)

    data_r = dict(data, oracle_reps=rng.normal(size=(len(data['terminals']), 2)).astype(np.float32))
    np.random.seed(202)
    record(out, 'reps', data_r, dsm.GCDataset(dsm.Dataset.create(**data_r), dict(REPS_CFG)), REPS_CFG)

    data_g = gv.regular_dataset(rng, (5,))
    np.random.seed(203)
    record(out, 'regular', data_g, dsm.GCDataset(dsm.Dataset.create(**data_g), dict(STATE_CFG)), STATE_CFG)

    data_v = gv.compact_dataset(rng, (6, 5, 2), np.uint8)
    np.random.seed(204)
    record(out, 'vis', data_v, dsm.GCDataset(dsm.Dataset.create(**data_v), dict(VIS_CFG),
                                             preprocess_frame_stack=False), VIS_CFG)

    path = os.path.join(OUT, 'trl_golden.npz')
    np.savez_compressed(path, **out)
    print('trl golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
