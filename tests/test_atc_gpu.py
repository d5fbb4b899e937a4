"""GPU tests of ATC batches (atc_sample_kernel via ogbx_atc_sample,
include/ogbx_atc.h): bit-exact against the reference's recorded batches with
injected draws (tests/golden/atc_golden.npz) and against the NumPy restatement
(tests/atc_np.py) replaying the kernel's own draws."""

import ctypes
import os

import numpy as np
import pytest
import torch

import atc_np as anp
from ogbench_amd import _lib
from ogbench_amd import datasets as D
from ogbench_amd.datasets import ATCDataset, Dataset

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'atc_golden.npz')
TAG_ATC_SAMPLE = 0x41540001  # common.h kTagAtcSample
CROP_SLOT = 8  # OGBX_VISUAL_CROP_SLOT
VIS_CFG = dict(frame_stack=3, p_aug=1.0)
NO_AUG = dict(frame_stack=None, p_aug=None)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _np(t):
    return t.cpu().numpy()


def _sampler(data, cfg, gpu, seed=1, **kw):
    return ATCDataset(Dataset(data, device=gpu), dict(cfg), seed=seed, **kw)


def _assert_batch(out, exp):
    assert [k for k in out if not k.startswith('_')] == list(anp.KEYS)
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (k, got.dtype, got.shape, v.dtype, v.shape)
        np.testing.assert_array_equal(got, v, err_msg=k)


def _replay(data, cfg, k, out):
    """The batch the restatement builds from `out`'s recorded draws."""
    draws = {key: _np(v) for key, v in out['_draws'].items()}
    crop_from = draws.pop('crop_from', None)
    exp, idxs = anp.batch(data, cfg, k, draws, crop_from)
    np.testing.assert_array_equal(_np(out['_idxs']), idxs)
    return exp, draws['pick'], crop_from


def _equal_trajectories(n_traj, length, frame_shape=(3,), dtype=np.float32, valids=True, seed=0):
    rng = np.random.RandomState(seed)
    R = n_traj * length
    term = np.zeros(R, np.float32)
    term[length - 1::length] = 1
    if dtype == np.uint8:
        obs = rng.randint(0, 256, (R,) + frame_shape).astype(np.uint8)
    else:
        obs = rng.normal(size=(R,) + frame_shape).astype(dtype)
    data = dict(observations=obs, terminals=term)
    if valids:
        data['valids'] = 1.0 - term
    return data


# ------------------------------------------------------------------------- 1
@pytest.mark.parametrize('case', list(anp.CASES))
def test_fixture_parity_with_injected_draws(gpu, gold, case):
    cfg, k = anp.CASES[case]
    data, _, valid, idxs, draws, exp, keys = anp.fixture_case(gold, case)
    s = _sampler(data, cfg, gpu, preprocess_frame_stack=case in anp.PREPROCESSED)
    out = s.sample(64, k, draws=draws, record_draws=True)
    assert [key for key in out if not key.startswith('_')] == keys
    _assert_batch(out, exp)
    np.testing.assert_array_equal(_np(out['_idxs']), idxs)
    np.testing.assert_array_equal(_np(out['_draws']['pick']), draws['pick'])
    assert ('crop_from' in out['_draws']) == ('crop_from' in draws)
    if 'crop_from' in draws:
        np.testing.assert_array_equal(_np(out['_draws']['crop_from']), draws['crop_from'])
    assert s._valid_k(k)[1] == len(valid)
    # the frames stay unstacked in HBM
    assert tuple(s.dataset['observations'].shape) == data['observations'].shape


# ------------------------------------------------------------------------- 2
@pytest.mark.parametrize('kind', ['compact', 'regular', 'mask'])
def test_valid_idxs_entry_point(gpu, gold, kind):
    data = dict(anp.fixture_case(gold, 'regular' if kind == 'regular' else 'vis')[0])
    if kind == 'mask':
        data['valids'] = (np.random.RandomState(4).rand(len(data['terminals'])) < 0.6).astype(np.float32)
        assert 0 < data['valids'].sum() < len(data['valids'])
    s = _sampler(data, NO_AUG, gpu)
    assert s.period[0] == 0
    for k in (0, 1, 2, 3, 16, 24, 29):
        want = anp.valid_idxs(data, k)
        table, n = s._valid_k(k)
        assert n == len(want), k
        got = _np(table) if table is not None else np.zeros(0, np.int64)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want, err_msg=str(k))
        assert table is None or table.untyped_storage().nbytes() == 8 * n  # a table of its own size
    calls = s._calls
    with pytest.raises(ValueError, match=r'^No valid ATC indices found for k=30\.$'):
        s.sample(8, 30)
    with pytest.raises(ValueError):
        s.sample(8, -1)
    assert s._calls == calls  # refused on the host, before any sample launch


def test_table_cache_is_bounded_and_lru(gpu, gold):
    data = anp.fixture_case(gold, 'state')[0]
    s = _sampler(data, NO_AUG, gpu)
    assert ATCDataset.TABLE_CACHE == 16
    s.TABLE_CACHE = 3
    for k in range(5):
        s.sample(4, k)
    assert list(s._tables) == [2, 3, 4]
    s.sample(4, 2)
    s.sample(4, 5)
    assert list(s._tables) == [4, 2, 5]
    np.testing.assert_array_equal(_np(s._tables[2][0]), anp.valid_idxs(data, 2))


# ------------------------------------------------------------------------- 3
@pytest.mark.parametrize('valids', [True, False])
def test_periodic_closed_form_equals_the_table_path(gpu, valids):
    data = _equal_trajectories(12, 9, valids=valids)
    closed = _sampler(data, NO_AUG, gpu, seed=77)
    table = _sampler(data, NO_AUG, gpu, seed=77, _periodic=False)
    assert closed.period == ((9, 8, 8) if valids else (9, 9, 8)) and table.period == (0, 0, 0)
    for k in (0, 1, 7, 8):
        a = closed.sample(257, k, record_draws=True)
        b = table.sample(257, k, record_draws=True)
        want = anp.valid_idxs(data, k)
        assert closed._valid_k(k) == (None, len(want)) and table._valid_k(k)[1] == len(want)
        assert torch.equal(a['_idxs'], b['_idxs']) and torch.equal(a['_draws']['pick'], b['_draws']['pick'])
        np.testing.assert_array_equal(_np(a['_idxs']), want[_np(a['_draws']['pick'])])
        for key in anp.KEYS:
            assert torch.equal(a[key], b[key]), (k, key)
        exp, _, _ = _replay(data, NO_AUG, k, a)
        _assert_batch(a, exp)
    assert closed._tables == {} and sorted(table._tables) == [0, 1, 7, 8]  # the closed form holds no table
    for s in (closed, table):
        with pytest.raises(ValueError, match=r'^No valid ATC indices found for k=9\.$'):
            s.sample(16, 9)


# ------------------------------------------------------------------------- 4
def test_philox_path_replays(gpu, gold):
    from oracle import locomaze as orc

    cfg, k = anp.CASES['vis']
    data = anp.fixture_case(gold, 'vis')[0]
    valid = anp.valid_idxs(data, k)
    seed = 12345678901234567
    a, b = (_sampler(data, cfg, gpu, seed=seed) for _ in range(2))
    k0, k1 = orc.philox_key(seed, TAG_ATC_SAMPLE)
    outs = []
    for call, B in enumerate((64, 67)):
        out = a.sample(B, k, record_draws=True)
        assert np.isin(_np(out['_idxs']), valid).all()
        exp, pick, cf = _replay(data, cfg, k, out)
        _assert_batch(out, exp)
        assert cf.shape == (B, 2) and cf.min() >= 0 and cf.max() <= 8
        # pick: slot 0, words x, y; crop: slot OGBX_VISUAL_CROP_SLOT, words x, y (ogbx_atc.h)
        for s in range(0, B, 5):
            w = orc.philox4x32([s, call, 0, 0], k0, k1)
            assert pick[s] == ((((int(w[0]) << 32) | int(w[1])) * len(valid)) >> 64), s
            w = orc.philox4x32([s, call, CROP_SLOT, 0], k0, k1)
            assert cf[s].tolist() == [(int(w[0]) * 9) >> 32, (int(w[1]) * 9) >> 32], s
        again = b.sample(B, k, record_draws=True)
        for key in anp.KEYS + ('_idxs',):
            assert torch.equal(out[key], again[key]), key
        outs.append(out)
    assert not np.array_equal(_np(outs[0]['_idxs']), _np(outs[1]['_idxs'])[:64])


def test_philox_picks_cover_valid_k(gpu, gold):
    """valid(3) of the fixture's compact layout has 70 rows; 65,536 uniform
    picks miss one of them with probability 70 (69/70)^65536 < 1e-400."""
    data = anp.fixture_case(gold, 'state')[0]
    valid = anp.valid_idxs(data, 3)
    assert len(valid) == 70
    out = _sampler(data, NO_AUG, gpu, seed=5).sample(65536, 3, record_draws=True)
    idxs = _np(out['_idxs'])
    assert sorted(set(idxs.tolist())) == valid.tolist()
    np.testing.assert_array_equal(_np(out['observations']), data['observations'][idxs])
    np.testing.assert_array_equal(_np(out['positive_observations']), data['observations'][idxs + 3])


# ------------------------------------------------------------------------- 5
def test_the_coin(gpu, gold):
    data = anp.fixture_case(gold, 'vis')[0]
    cfg = dict(VIS_CFG, p_aug=0.5)
    s = _sampler(data, cfg, gpu, seed=3)
    np.random.seed(11)
    state = np.random.get_state()
    ev = s.sample(32, 2, evaluation=True, record_draws=True)
    assert 'crop_from' not in ev['_draws']
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    exp, _, _ = _replay(data, cfg, 2, ev)
    _assert_batch(ev, exp)
    cropped = []
    for _ in range(12):
        out = s.sample(32, 2, record_draws=True)
        cropped.append('crop_from' in out['_draws'])
        exp, _, _ = _replay(data, cfg, 2, out)
        _assert_batch(out, exp)
    np.random.seed(11)
    want = [bool(np.random.rand() < 0.5) for _ in range(12)]
    assert cropped == want and True in want and False in want
    # p_aug None or 0: no coin
    for p in (None, 0.0):
        np.random.seed(12)
        state = np.random.get_state()
        _sampler(data, dict(cfg, p_aug=p), gpu, seed=3).sample(8, 2)
        assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]


# ------------------------------------------------------------------------- 6
def test_out_refills_in_place(gpu, gold):
    data = anp.fixture_case(gold, 'vis')[0]
    a, b = (_sampler(data, VIS_CFG, gpu, seed=21) for _ in range(2))
    first = a.sample(64, 2)
    assert list(first) == list(anp.KEYS)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    snap = {k: v.clone() for k, v in first.items()}
    second = a.sample(64, 2, out=first)
    assert second is first and {k: v.data_ptr() for k, v in second.items()} == ptrs
    b.sample(64, 2)
    want = b.sample(64, 2)
    for k, v in want.items():
        assert torch.equal(second[k], v), k
    assert not torch.equal(second['observations'], snap['observations'])
    # another k on the refill
    third = a.sample(64, 5, out=first)
    want = b.sample(64, 5, record_draws=True)
    assert third is first and {k: v.data_ptr() for k, v in third.items()} == ptrs
    for k in anp.KEYS:
        assert torch.equal(third[k], want[k]), k
    exp, _, _ = _replay(data, VIS_CFG, 5, want)
    _assert_batch(third, exp)


def test_replaced_observations_are_noticed(gpu, gold):
    data = anp.fixture_case(gold, 'state')[0]
    a, b = (_sampler(data, NO_AUG, gpu, seed=9) for _ in range(2))
    first = a.sample(16, 1)
    new = data['observations'] + 1
    a.dataset['observations'] = torch.as_tensor(new, device=gpu)
    out = a.sample(16, 1, out=first)
    b.sample(16, 1)
    ref = b.sample(16, 1, record_draws=True)
    exp, _, _ = _replay(dict(data, observations=new), NO_AUG, 1, ref)
    _assert_batch(out, exp)
    a.dataset['observations'] = torch.zeros(3, 5, device=gpu)
    with pytest.raises(ValueError, match='changed shape'):
        a.sample(16, 1)


# ------------------------------------------------------------------------- 7
def test_explicit_idxs(gpu, gold):
    cfg, k = anp.CASES['vis']
    data, _, valid, idxs, draws, exp, _ = anp.fixture_case(gold, 'vis')
    s = _sampler(data, cfg, gpu, seed=2)
    out = s.sample(64, k, idxs=idxs, draws=dict(crop_from=draws['crop_from']), record_draws=True)
    _assert_batch(out, exp)
    np.testing.assert_array_equal(_np(out['_idxs']), idxs)
    assert (_np(out['_draws']['pick']) == -1).all()
    # rows whose idx + k passes the trajectory end, the buffer's last row and rows outside it among them
    last = np.nonzero(data['terminals'] > 0)[0]
    bad = idxs.copy()
    bad[[3, 40, 63]] = [last[0], last[-1] - 1, last[-1]]
    with pytest.raises(ValueError, match=r'\b3 of 64 samples'):
        s.sample(64, k, idxs=bad)
    bad[[0, 1]] = [-1, len(data['terminals'])]
    with pytest.raises(ValueError, match=r'\b5 of 64 samples'):
        s.sample(64, k, idxs=bad)
    # the sampler still works
    out = s.sample(64, k, idxs=idxs, draws=dict(crop_from=draws['crop_from']))
    _assert_batch(out, exp)


def test_non_device_pointer_is_refused(gpu, gold):
    """A host pointer among the outputs: OGBX_EINVAL before any launch."""
    data = anp.fixture_case(gold, 'state')[0]
    s = _sampler(data, NO_AUG, gpu)
    batch, col = s._batch(8)  # `batch` keeps the column's destinations alive
    table, n = s._valid_k(1)
    host = (ctypes.c_int64 * 8)()
    outs = D.AtcOutputs(ctypes.addressof(host), None, None, None)
    st = s._L.ogbx_atc_sample(s._buf, col, 8, 1, _lib.ptr(table), n, 1, 4, None, None, None, 0, 1, 0, outs, None)
    assert st == _lib.OGBX_EINVAL and 'device memory' in _lib.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------- 8
def test_band_path(gpu):
    """uint8 frames 72 x 80 x 3 stacked 8 deep: 138,240 B of stack, over the
    64 KB of LDS, so the output is composed band by band."""
    data = _equal_trajectories(4, 12, (72, 80, 3), np.uint8, seed=6)
    cfg = dict(frame_stack=8, p_aug=1.0)
    s = _sampler(data, cfg, gpu, seed=8)
    out = s.sample(7, 2, record_draws=True)
    exp, _, cf = _replay(data, cfg, 2, out)
    assert cf is not None and out['observations'].shape == (7, 72, 80, 24)
    _assert_batch(out, exp)


def test_float_frames_without_stack(gpu):
    """float32 4-D observations (12-byte pixels), crop only, ragged trajectories."""
    rng = np.random.RandomState(7)
    lengths = [5, 2, 11, 3]
    R = sum(lengths)
    term = np.zeros(R, np.float32)
    term[np.cumsum(lengths) - 1] = 1
    data = dict(observations=rng.normal(size=(R, 5, 7, 3)).astype(np.float32), terminals=term, valids=1.0 - term)
    cfg = dict(frame_stack=None, p_aug=1.0, augment_padding=2)
    s = _sampler(data, cfg, gpu, seed=4)
    out = s.sample(33, 1, record_draws=True)
    exp, _, cf = _replay(data, cfg, 1, out)
    assert cf.min() >= 0 and cf.max() <= 4 and len({tuple(c) for c in cf.tolist()}) > 5
    _assert_batch(out, exp)
