"""GPU tests of visual batches: frame stack and random crop of GCDataset /
HGCDataset (visual_gather_kernel via ogbx_visual_gather), bit-exact against the
reference's recorded batches with injected draws and against the NumPy
restatement (tests/visual_np.py) replaying the kernel's own draws."""

import os

import numpy as np
import pytest
import torch

import visual_np as vnp
from ogbench_amd.datasets import Dataset, GCDataset, HGCDataset

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'visual_golden.npz')
PLAIN = dict(frame_stack=None, p_aug=None)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope='module')
def frames64():
    """About 2,000 rows of 64 x 64 x 3 uint8 frames in ragged trajectories
    (some shorter than the stack), compact layout."""
    rng = np.random.RandomState(7)
    lengths = [2, 3, 150, 1, 97, 200] * 4 + [188]
    R = sum(lengths)
    term = np.zeros(R, np.float32)
    term[np.cumsum(lengths) - 1] = 1
    return dict(observations=rng.randint(0, 256, (R, 64, 64, 3)).astype(np.uint8),
                actions=rng.uniform(-1, 1, (R, 4)).astype(np.float32), terminals=term, valids=1.0 - term)


def _np(t):
    return t.cpu().numpy()


def _sampler(data, cfg, gpu, hgc=False, seed=1):
    return (HGCDataset if hgc else GCDataset)(Dataset(data, device=gpu), dict(cfg), seed=seed)


def _replay(data, cfg, out, hgc):
    """The image keys of `out` from its recorded indices and crop offsets."""
    R = len(data['observations'])
    tend = vnp.traj_end(data['terminals'])
    if hgc:
        lvg = _np(out['_low_value_goal_idxs'])
        sel = vnp.hgc_selectors(_np(out['_idxs']), _np(out['_high_value_goal_idxs']),
                                _np(out['_high_actor_goal_idxs']), lvg, tend, R, *vnp.hgc_steps(cfg))
    else:
        sel = vnp.gc_selectors(_np(out['_idxs']), _np(out['_value_goal_idxs']), _np(out['_actor_goal_idxs']), R)
    cf = out['_draws'].get('crop_from')
    return vnp.visual_batch(data, sel, cfg['frame_stack'], _np(cf) if cf is not None else None, hgc=hgc,
                            has_low=cfg.get('low_discount') is not None)


def _assert_images(out, exp):
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (k, got.shape, v.shape)
        assert np.array_equal(got, v), k


@pytest.mark.parametrize('case', list(vnp.CASES))
def test_fixture_parity_with_injected_draws(gpu, gold, case):
    cfg, hgc, evaluation = vnp.CASES[case]
    data, draws, exp = vnp.fixture_case(gold, case)
    s = _sampler(data, cfg, gpu, hgc)
    out = s.sample(len(draws['pick']), draws=draws, evaluation=evaluation)
    assert set(exp) <= set(out)
    _assert_images(out, exp)
    # the frames stay unstacked in HBM
    assert tuple(s.dataset['observations'].shape) == data['observations'].shape
    if case == 'E':
        sel0 = _np(s.dataset.valid_idxs)[draws['pick']]
        uncropped = vnp.stacked(data['observations'], sel0, vnp.traj_end(data['terminals']), 3)
        assert np.array_equal(_np(out['high_value_reps']), uncropped)
        assert not np.array_equal(_np(out['observations']), uncropped)  # observations are cropped
        assert np.array_equal(_np(out['low_value_goals']), exp['low_value_goals'])
        cropped = vnp.crop(exp['low_value_goals'], draws['crop_from'])
        assert not np.array_equal(cropped, exp['low_value_goals'])  # a crop would have shown
        assert torch.equal(out['value_goals'], out['high_value_goals'])


@pytest.mark.parametrize('hgc', [False, True])
def test_philox_draws_replay_and_leave_other_keys_alone(gpu, gold, hgc):
    cfg = vnp.HGC_CFG if hgc else vnp.GC_CFG
    data, _, _ = vnp.fixture_case(gold, 'A')
    vis, again, plain = (_sampler(data, c, gpu, hgc, seed=11) for c in (cfg, cfg, dict(cfg, **PLAIN)))
    for kw in (dict(batch_size=67), dict(batch_size=256, num_batches=2)):
        out = vis.sample(record_draws=True, **kw)
        total = kw['batch_size'] * kw.get('num_batches', 1)
        cf = _np(out['_draws']['crop_from'])
        assert cf.shape == (total, 2) and cf.min() >= 0 and cf.max() <= 6
        images = _replay(data, cfg, out, hgc)
        _assert_images(out, images)
        # the same seed and call give the same batch
        out2 = again.sample(record_draws=True, **kw)
        for k, v in out.items():
            if k != '_draws':
                assert torch.equal(v, out2[k]), k
        assert torch.equal(out['_draws']['crop_from'], out2['_draws']['crop_from'])
        # every other key, the indices and the shared draws are the non-visual sampler's
        ref = plain.sample(record_draws=True, **kw)
        for k, v in ref.items():
            if k == '_draws':
                for d, t in v.items():
                    assert torch.equal(out['_draws'][d], t), d
            elif k not in images:
                assert torch.equal(out[k], v), k
        assert 'crop_from' not in ref['_draws']


def test_philox_offsets_cover_the_window(gpu, gold):
    """4,096 samples: each of the 49 offset pairs occurs (a fair draw misses
    one with probability about 49 exp(-84))."""
    data, _, _ = vnp.fixture_case(gold, 'A')
    out = _sampler(data, vnp.GC_CFG, gpu, seed=3).sample(4096, record_draws=True)
    cf = _np(out['_draws']['crop_from'])
    assert cf.min() >= 0 and cf.max() <= 6
    assert len({tuple(c) for c in cf.tolist()}) == 49
    _assert_images(out, _replay(data, vnp.GC_CFG, out, False))


def test_no_crop_call_records_no_offsets(gpu, gold):
    data, _, _ = vnp.fixture_case(gold, 'A')
    out = _sampler(data, vnp.GC_CFG, gpu, seed=3).sample(32, record_draws=True, evaluation=True)
    assert 'crop_from' not in out['_draws']
    _assert_images(out, _replay(data, vnp.GC_CFG, out, False))


def test_stack_of_one_equals_the_fused_path(gpu, frames64):
    cfg = dict(vnp.GC_CFG, p_aug=0.5)
    vis = _sampler(frames64, dict(cfg, frame_stack=1), gpu, seed=5)
    plain = _sampler(frames64, dict(cfg, **PLAIN), gpu, seed=5)
    out, ref = vis.sample(256, evaluation=True), plain.sample(256, evaluation=True)
    assert set(out) == set(ref)
    for k, v in ref.items():
        assert torch.equal(out[k], v), k


def test_realistic_shape_against_restatement(gpu, frames64):
    out = _sampler(frames64, vnp.GC_CFG, gpu, seed=9).sample(256, record_draws=True)
    assert tuple(out['observations'].shape) == (256, 64, 64, 9)
    assert len({tuple(c) for c in _np(out['_draws']['crop_from']).tolist()}) > 40
    _assert_images(out, _replay(frames64, vnp.GC_CFG, out, False))


def test_banded_staging_of_large_frames(gpu):
    """Four 80 x 72 x 3 frames (69 KB) exceed the 64-KB staging budget: the
    kernel stages bands of rows; 216-byte rows are 8- but not 16-byte aligned."""
    rng = np.random.RandomState(1)
    lengths = [2, 30, 3, 21]
    R = sum(lengths)
    term = np.zeros(R, np.float32)
    term[np.cumsum(lengths) - 1] = 1
    data = dict(observations=rng.randint(0, 256, (R, 80, 72, 3)).astype(np.uint8),
                actions=rng.uniform(-1, 1, (R, 2)).astype(np.float32), terminals=term, valids=1.0 - term)
    cfg = dict(vnp.GC_CFG, frame_stack=4)
    out = _sampler(data, cfg, gpu, seed=2).sample(24, record_draws=True)
    _assert_images(out, _replay(data, cfg, out, False))


def test_oracle_reps_goals_are_neither_stacked_nor_cropped(gpu, gold):
    data, _, _ = vnp.fixture_case(gold, 'A')
    data = dict(data, oracle_reps=np.arange(2 * len(data['terminals']), dtype=np.float32).reshape(-1, 2))
    out = _sampler(data, vnp.GC_CFG, gpu, seed=4).sample(64, record_draws=True)
    assert np.array_equal(_np(out['value_goals']), data['oracle_reps'][_np(out['_value_goal_idxs'])])
    assert np.array_equal(_np(out['actor_goals']), data['oracle_reps'][_np(out['_actor_goal_idxs'])])
    images = _replay(data, vnp.GC_CFG, out, False)
    assert set(images) == {'observations', 'next_observations'}
    _assert_images(out, images)


def test_out_refills_in_place(gpu, gold):
    data, _, _ = vnp.fixture_case(gold, 'B')
    a, b = (_sampler(data, vnp.GC_CFG, gpu, seed=21) for _ in range(2))
    first = a.sample(64)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    snap = {k: v.clone() for k, v in first.items()}
    second = a.sample(64, out=first)
    assert second is first and {k: v.data_ptr() for k, v in second.items()} == ptrs
    b.sample(64)
    want = b.sample(64)
    for k, v in want.items():
        assert torch.equal(second[k], v), k
    assert not torch.equal(second['observations'], snap['observations'])


def test_frame_stack_needs_a_compact_dataset(gpu, gold):
    data, _, _ = vnp.fixture_case(gold, 'F')
    with pytest.raises(AssertionError):
        _sampler(data, vnp.GC_CFG, gpu)


def test_bad_crop_from_shape_raises(gpu, gold):
    data, draws, _ = vnp.fixture_case(gold, 'A')
    s = _sampler(data, vnp.GC_CFG, gpu)
    with pytest.raises(ValueError, match='crop_from'):
        s.sample(64, draws=dict(draws, crop_from=draws['crop_from'][:, :1]))
    with pytest.raises(ValueError, match='crop_from'):
        s.sample(64, draws=dict(draws, crop_from=draws['crop_from'][:32]))
