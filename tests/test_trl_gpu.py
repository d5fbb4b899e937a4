"""GPU tests of TRL batches of GCDataset (trl_sample_kernel via ogbx_trl_sample,
include/ogbx_trl.h): bit-exact against the reference's recorded batches with
injected draws (tests/golden/trl_golden.npz) and against the NumPy restatement
(tests/trl_np.py) replaying the kernel's own draws."""

import ctypes
import os

import numpy as np
import pytest
import torch

import trl_np as tnp
import visual_np as vnp
from ogbench_amd import _lib
from ogbench_amd import datasets as D
from ogbench_amd.datasets import Dataset, GCDataset, HGCDataset

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'trl_golden.npz')
GC_KEYS = ('observations', 'actions', 'terminals', 'valids', 'next_observations', 'value_goals', 'actor_goals',
           'masks', 'rewards')
TAG_GC_SAMPLE = 0x47430001  # common.h kTagGcSample


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _np(t):
    return t.cpu().numpy()


def _sampler(data, cfg, gpu, seed=1):
    return GCDataset(Dataset(data, device=gpu), dict(cfg), seed=seed)


def _assert_batch(out, exp, keys=None):
    if keys is not None:
        assert [k for k in out if not k.startswith('_')] == list(keys)
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (k, got.dtype, got.shape, v.dtype, v.shape)
        np.testing.assert_array_equal(got, v, err_msg=k)


def _replay(data, cfg, out):
    """The batch the restatement builds from `out`'s recorded draws."""
    draws = {k: _np(v) for k, v in out['_draws'].items()}
    crop_from = draws.pop('crop_from', None)
    exp, ix = tnp.batch(data, cfg, draws, crop_from)
    np.testing.assert_array_equal(_np(out['_idxs']), ix['idxs'])
    np.testing.assert_array_equal(_np(out['_value_goal_idxs']), ix['vg'])
    np.testing.assert_array_equal(_np(out['_actor_goal_idxs']), ix['ag'])
    np.testing.assert_array_equal(_np(out['_value_midpoint_idxs']), ix['mid'])
    return exp, ix


def _equal_trajectories(n_traj, length, seed=0):
    rng = np.random.RandomState(seed)
    R = n_traj * length
    term = np.zeros(R, np.float32)
    term[length - 1::length] = 1
    return dict(observations=rng.normal(size=(R, 3)).astype(np.float32),
                actions=rng.uniform(-1, 1, (R, 2)).astype(np.float32), terminals=term, valids=1.0 - term)


# ------------------------------------------------------------------------ T3
@pytest.mark.parametrize('case', list(tnp.CASES))
def test_fixture_parity_with_injected_draws(gpu, gold, case):
    cfg = tnp.CASES[case]
    data, draws, exp, keys = tnp.fixture_case(gold, case)
    s = _sampler(data, cfg, gpu)
    out = s.sample(len(draws['pick']), draws=draws)
    _assert_batch(out, exp, keys)
    assert out['value_offsets'].dtype == torch.int64 and out['value_midpoint_offsets'].dtype == torch.int64
    # one tensor where the reference computes one expression twice
    assert out['actor_goal_observations'] is out['value_goal_observations']
    if 'oracle_reps' not in data:
        assert out['value_cur_goals'] is out['observations']
        assert out['value_midpoint_goals'] is out['value_midpoint_observations']
        if 'next_observations' not in data:
            assert out['value_next_goals'] is out['next_observations']
    else:
        assert out['value_goals'] is not out['value_goal_observations']
        assert out['value_goals'].shape != out['value_goal_observations'].shape
        assert out['value_midpoint_goals'] is not out['value_midpoint_observations']
    # the frames stay unstacked in HBM
    assert tuple(s.dataset['observations'].shape) == data['observations'].shape


# ------------------------------------------------------------------------ T4
def test_philox_path_matches_the_gc_sampler_and_replays(gpu, gold):
    from oracle import locomaze as orc

    cfg = tnp.CASES['state']
    data, _, _, keys = tnp.fixture_case(gold, 'state')
    table = tnp.pick_table(data['terminals'])
    valids = np.zeros(len(data['terminals']), np.float32)
    valids[table] = 1  # the TRL rows as the plain sampler's pick table
    plain_cfg = {k: v for k, v in cfg.items() if k != 'agent_name'}
    seed = 12345678901234567
    trl = _sampler(data, cfg, gpu, seed=seed)
    plain = _sampler(dict(data, valids=valids), plain_cfg, gpu, seed=seed)
    k0, k1 = orc.philox_key(seed, TAG_GC_SAMPLE)
    for call, kw in enumerate((dict(batch_size=64), dict(batch_size=67, num_batches=2))):
        out = trl.sample(record_draws=True, **kw)
        ref = plain.sample(record_draws=True, **kw)
        for k in ('_idxs', '_value_goal_idxs', '_actor_goal_idxs') + GC_KEYS:
            assert torch.equal(out[k], ref[k]), k
        for k, v in ref['_draws'].items():
            assert torch.equal(out['_draws'][k], v), k
        exp, ix = _replay(data, cfg, out)
        _assert_batch(out, exp, keys)
        assert torch.equal(out['_draws']['midpoint'], out['_value_midpoint_idxs'])
        # the midpoint takes words z, w of Philox slot 4 (ogbx_trl.h)
        for s in range(0, len(ix['idxs']), 5):
            w = orc.philox4x32([s, call, 4, 0], k0, k1)
            u = (int(w[2]) << 32) | int(w[3])
            span = int(ix['vg'][s] - ix['idxs'][s])
            assert ix['mid'][s] == ix['idxs'][s] + ((u * span) >> 64), s


# ------------------------------------------------------------------------ T5
def test_midpoint_covers_its_range(gpu):
    """64 trajectories of 5 rows, discount 0.5, geometric value goals, 4,096
    samples at seed 99, call 0.  The sample chain restated on the CPU (Philox
    slots 0 and 1 through the oracle's philox4x32: pick, geometric offset,
    span = min(offset, rows left)) counts 2,549 / 1,038 / 365 / 144 samples
    with span 1 / 2 / 3 / 4 (expected 2,560 / 1,024 / 384 / 128); the kernel
    must give the same counts, and an honest uniform draw then misses one of a
    span's offsets with probability at most
    2 (1/2)^1038 + 3 (2/3)^365 + 4 (3/4)^144 = 4e-18 < 1e-12."""
    data = _equal_trajectories(64, 5)
    cfg = dict(tnp.STATE_CFG, discount=0.5)
    out = _sampler(data, cfg, gpu, seed=99).sample(1024, num_batches=4, record_draws=True)
    exp, ix = _replay(data, cfg, out)
    idx, mid, vg = ix['idxs'], ix['mid'], ix['vg']
    assert len(idx) == 4096
    assert (idx <= mid).all() and (mid < vg).all()
    span, off = vg - idx, mid - idx
    np.testing.assert_array_equal(_np(out['value_offsets']), span)
    np.testing.assert_array_equal(_np(out['value_midpoint_offsets']), off)
    counts = {n: int((span == n).sum()) for n in (1, 2, 3, 4)}
    print('samples per span:', counts)
    assert counts == {1: 2549, 2: 1038, 3: 365, 4: 144}
    assert sum(n * ((n - 1) / n) ** counts[n] for n in (2, 3, 4)) < 1e-12
    for n in (2, 3, 4):
        assert set(off[span == n].tolist()) == set(range(n)), n
    assert (off[span == 1] == 0).all()


# ------------------------------------------------------------------------ T6
@pytest.mark.parametrize('form', ['valid_pairs', 'periodic', 'explicit_idxs'])
def test_tile_and_batch_edges(gpu, gold, form):
    cfg = tnp.CASES['state']
    if form == 'periodic':
        data = _equal_trajectories(12, 7, seed=3)
    else:
        data = tnp.fixture_case(gold, 'state')[0]
    s = _sampler(data, cfg, gpu, seed=5)
    assert (s._buf.period > 0) == (form == 'periodic')
    assert s._buf.valid_pairs
    table = tnp.pick_table(data['terminals'])
    rng = np.random.RandomState(8)
    for B, nb in ((1, 1), (63, 1), (65, 1), (129, 1), (65, 2)):
        idxs = table[rng.randint(0, len(table), B * nb)] if form == 'explicit_idxs' else None
        out = s.sample(B, num_batches=nb, idxs=idxs, record_draws=True)
        draws = {k: _np(v) for k, v in out['_draws'].items()}
        exp, ix = tnp.batch(data, cfg, draws, idxs=idxs)
        assert len(ix['idxs']) == B * nb
        if idxs is not None:
            np.testing.assert_array_equal(_np(out['_idxs']), idxs)
        np.testing.assert_array_equal(_np(out['_value_goal_idxs']), ix['vg'])
        np.testing.assert_array_equal(_np(out['_value_midpoint_idxs']), ix['mid'])
        assert (ix['idxs'] <= ix['mid']).all() and (ix['mid'] < ix['vg']).all()
        _assert_batch(out, exp)


# ------------------------------------------------------------------------ T7
def test_explicit_last_rows_raise_with_their_count(gpu, gold):
    data = tnp.fixture_case(gold, 'state')[0]
    s = _sampler(data, tnp.CASES['state'], gpu, seed=2)
    table = tnp.pick_table(data['terminals'])
    last = np.nonzero(data['terminals'] > 0)[0]
    idxs = table[:64].copy()
    idxs[[3, 40, 63]] = last[[0, 4, len(last) - 1]]  # the very last row of the buffer among them
    with pytest.raises(ValueError, match=r'\b3 of 64 samples'):
        s.sample(64, idxs=idxs)
    # the sampler still works, and good explicit rows pass
    out = s.sample(64, idxs=table[:64], record_draws=True)
    np.testing.assert_array_equal(_np(out['_idxs']), table[:64])
    # an injected value goal at the sample itself is counted too
    draws = {k: _np(v) for k, v in out['_draws'].items()}
    draws['v_geom'] = draws['v_geom'].copy()
    draws['v_geom'][:2] = 0
    with pytest.raises(ValueError, match=r'\b2 of 64 samples'):
        s.sample(64, idxs=table[:64], draws=draws)


def test_non_device_pointer_is_refused(gpu, gold):
    """A host pointer among the outputs: OGBX_EINVAL before any launch."""
    data = tnp.fixture_case(gold, 'state')[0]
    s = _sampler(data, tnp.CASES['state'], gpu)
    host = (ctypes.c_double * 64)()
    ok = torch.empty(64, dtype=torch.float64, device=gpu)
    outs = D.TrlOutputs(None, None, None, None, None, None, ok.data_ptr(), ctypes.addressof(host), None)
    st = s._L.ogbx_trl_sample(s._buf, s._cfg, None, 0, 64, 1, None, None, 1, 0, outs, None, None, None)
    assert st == _lib.OGBX_EINVAL and 'device memory' in _lib.last_error()
    torch.cuda.synchronize()


def test_valid_idxs_entry_point(gpu, gold):
    data = tnp.fixture_case(gold, 'regular')[0]
    s = _sampler(data, tnp.CASES['regular'], gpu)
    np.testing.assert_array_equal(_np(s._valid), tnp.pick_table(data['terminals']))
    assert not hasattr(s.dataset, 'valid_idxs')


# ------------------------------------------------------------------------ T8
def test_construction(gpu, gold):
    data = tnp.fixture_case(gold, 'state')[0]
    cfg = tnp.CASES['state']
    with pytest.raises(ValueError, match='value_p_randomgoal'):
        _sampler(data, dict(cfg, value_p_trajgoal=0.5, value_p_randomgoal=0.5), gpu)
    with pytest.raises(ValueError, match='value_p_curgoal'):
        _sampler(data, dict(cfg, value_p_trajgoal=0.5, value_p_curgoal=0.5), gpu)
    for name in D.TRL_AGENTS:
        with pytest.raises(NotImplementedError):
            HGCDataset(Dataset(data, device=gpu), dict(cfg, agent_name=name, subgoal_steps=5))
        assert _sampler(data, dict(cfg, agent_name=name), gpu)._trl
    # the shared Dataset keeps its own pick table: compact data with one more
    # row invalid than the TRL table leaves out
    valids = data['valids'].copy()
    valids[5] = 0
    ds = Dataset(dict(data, valids=valids), device=gpu)
    held, before = ds.valid_idxs, ds.valid_idxs.clone()
    s = GCDataset(ds, dict(cfg), seed=1)
    assert ds.valid_idxs is held and torch.equal(held, before)
    assert s._valid.numel() == before.numel() + 1
    np.testing.assert_array_equal(_np(s._valid), tnp.pick_table(data['terminals']))


# ------------------------------------------------------------------------ T9
def test_out_refills_in_place(gpu, gold):
    data = tnp.fixture_case(gold, 'reps')[0]
    a, b = (_sampler(data, tnp.CASES['reps'], gpu, seed=21) for _ in range(2))
    first = a.sample(64)
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    snap = {k: v.clone() for k, v in first.items()}
    second = a.sample(64, out=first)
    assert second is first and {k: v.data_ptr() for k, v in second.items()} == ptrs
    b.sample(64)
    want = b.sample(64)
    assert list(want) == list(second)
    for k, v in want.items():
        assert torch.equal(second[k], v), k
    assert not torch.equal(second['value_midpoint_observations'], snap['value_midpoint_observations'])


# ----------------------------------------------------------------------- T10
def test_visual_philox_crops(gpu, gold):
    cfg = tnp.CASES['vis']
    data, _, _, keys = tnp.fixture_case(gold, 'vis')
    s = _sampler(data, cfg, gpu, seed=17)
    out = s.sample(67, num_batches=2, record_draws=True)
    cf = _np(out['_draws']['crop_from'])
    assert cf.shape == (134, 2) and cf.min() >= 0 and cf.max() <= 6 and len({tuple(c) for c in cf.tolist()}) > 20
    exp, ix = _replay(data, cfg, out)
    _assert_batch(out, exp, keys)
    # every cropped key of a sample has the sample's one offset pair: undoing
    # nothing, each equals the crop of its own uncropped stack at `cf`
    tend = vnp.traj_end(data['terminals'])
    rows = {'observations': ix['idxs'], 'next_observations': ix['idxs'] + 1, 'value_goals': ix['vg'],
            'actor_goals': ix['ag'], 'value_goal_observations': ix['vg'], 'value_midpoint_observations': ix['mid'],
            'value_midpoint_goals': ix['mid'], 'value_cur_goals': ix['idxs'], 'value_next_goals': ix['idxs'] + 1}
    for k, r in rows.items():
        plain = vnp.stacked(data['observations'], r, tend, 3)
        np.testing.assert_array_equal(_np(out[k]), vnp.crop(plain, cf), err_msg=k)
    assert not np.array_equal(_np(out['value_midpoint_observations']),
                              vnp.stacked(data['observations'], ix['mid'], tend, 3))
    # evaluation crops nothing
    ev = s.sample(64, record_draws=True, evaluation=True)
    assert 'crop_from' not in ev['_draws']
    exp, ix = _replay(data, cfg, ev)
    _assert_batch(ev, exp, keys)
    np.testing.assert_array_equal(_np(ev['value_midpoint_observations']),
                                  vnp.stacked(data['observations'], ix['mid'], tend, 3))
