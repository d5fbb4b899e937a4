"""GPU tests of ATC batches over the episode ring (ogbx_online_atc_table /
online_atc_sample_kernel via include/ogbx_online_atc.h,
ogbench_amd.datasets.GCReplayBuffer.sample_atc): bit for bit against the
reference's recorded behaviour (tests/golden/online_atc_golden.npz), the NumPy
restatement (tests/online_atc_np.py) and the offline ATCDataset over the
snapshot."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import atc_np as anp
import ogbench_amd
import online_atc_np as oan
import online_np as onp
import online_visual_np as ovn
from ogbench_amd import _lib, _online_atc
from ogbench_amd import datasets as D
from ogbench_amd.datasets import ATCDataset, Dataset, GCReplayBuffer, HGCReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_atc_golden.npz')
TILE = _online_atc.ONLINE_ATC_TABLE_TILE
GC_CFG = dict(onp.GOLDEN_CONFIGS['geom_neg'])
STATE = dict(GC_CFG, frame_stack=None, p_aug=None)
VIS = dict(GC_CFG, frame_stack=3, p_aug=1.0)
FORMS = {'vis': (VIS, np.zeros(ovn.FRAME, np.uint8)), 'state': (STATE, np.zeros(2))}
EX_STATE = dict(observations=np.zeros(2))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _np(t):
    return t.cpu().numpy()


def _assert_batch(out, exp, what=''):
    assert [k for k in out if not k.startswith('_')] == list(exp) == list(anp.KEYS), what
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (what, k, got.dtype, got.shape, v.dtype, v.shape)
        np.testing.assert_array_equal(got, v, err_msg=f'{what} {k}')


def _obs(rng, n, ex):
    v = np.array(ex['observations'])
    hi = 256 if v.dtype == np.uint8 else 100
    return dict(observations=rng.randint(0, hi, (n,) + v.shape).astype(v.dtype))


class Pair:
    """A GCReplayBuffer and its restatement, fed the same rows."""

    def __init__(self, N, T, cfg, gpu, seed=1, ex=EX_STATE, cls=GCReplayBuffer, start=None):
        self.buf = cls.create(ex, N, T, cfg, device=gpu, seed=seed)
        self.ref = onp.OnlineNp(ex, N, T)
        self.cfg, self.gpu, self.ex = cfg, gpu, ex
        if start is not None:  # the ordinals every env starts from
            first = np.array([start] * N, np.uint32).astype(np.int32)
            self.buf.cur_seq.copy_(torch.as_tensor(first))
            self.ref.cur_seq[:] = first

    def add(self, batch, done):
        self.buf.add({k: torch.as_tensor(v).to(self.gpu) for k, v in batch.items()}, torch.as_tensor(done).to(self.gpu))
        with np.errstate(over='ignore'):
            self.ref.add(batch, done)

    def fill(self, rng, steps, p):
        for _ in range(steps):
            self.add(_obs(rng, self.ref.N, self.ex), rng.rand(self.ref.N) < p)

    def check(self, B, k, what='', pick=None, idxs=None, crop_from=None, **kw):
        """One recording call with injected draws against the restatement."""
        draws = {}
        if pick is not None:
            draws['pick'] = pick
        if crop_from is not None:
            draws['crop_from'] = crop_from
        out = self.buf.sample_atc(B, k, idxs=idxs, draws=draws, record_draws=True, **kw)
        exp, ix = oan.batch(self.ref, self.cfg, k, dict(idxs=idxs) if idxs is not None else dict(pick=pick), crop_from)
        _assert_batch(out, exp, what)
        np.testing.assert_array_equal(_np(out['_idxs']), ix, err_msg=what)
        np.testing.assert_array_equal(_np(out['_draws']['pick']), pick if idxs is None else np.full(B, -1))
        return out


# ------------------------------------------------------------- the golden history
@pytest.mark.parametrize('form', list(FORMS))
def test_golden_history_samples_equal_the_reference(gpu, gold, form):
    cfg, example = FORMS[form]
    p = Pair(ovn.N, ovn.T, cfg, gpu, ex=dict(observations=example))
    builds = 0
    for t in range(ovn.STEPS):
        p.add(dict(observations=gold[f'{form}_in_observations'][t]), gold['done'][t])
        S = t + 1
        if S not in ovn.SNAPS:
            continue
        for k in (1, 2, 3):
            tag = f's{S}_k{k}_{form}'
            valid = gold[f's{S}_k{k}_valid']
            if len(valid) == 0:  # (3, 3): the reference's message, decided on the host
                assert (S, k) == (3, 3)
                with pytest.raises(ValueError) as err:
                    p.buf.sample_atc(64, k)
                assert str(err.value) == str(gold['s3_k3_error'])
                continue
            draws = dict(pick=gold[f'{tag}_draw_pick'])
            if form == 'vis':
                draws['crop_from'] = gold[f'{tag}_draw_crop_from']
            out = p.buf.sample_atc(64, k, draws=draws, record_draws=True)
            builds += 1
            keys = [str(x) for x in gold[f'{tag}_keys']]
            _assert_batch(out, {key: gold[f'{tag}_out_{key}'] for key in keys}, tag)
            np.testing.assert_array_equal(_np(out['_idxs']), gold[f'{tag}_idxs'])
            assert int(p.buf._atc_P[-1]) == len(valid)
            W, P = oan.table(p.ref, k)
            np.testing.assert_array_equal(_np(p.buf._atc_P), P)
    assert p.buf.atc_table_builds == builds == 11


# ------------------------------------------------ shapes where the kernels can go wrong
def _designed_done(step, N):
    """Env e closes an episode every 2 + e % 4 steps, staggered; e % 7 == 5
    never does (one open episode), e % 7 == 6 always (episodes of length 1)."""
    e = np.arange(N)
    done = (step + e) % (2 + e % 4) == 0
    done[e % 7 == 5] = False
    done[e % 7 == 6] = True
    return done


@pytest.mark.parametrize('N,T,start', [(1, 2, None), (3, 4, None), (3, 4, 0xFFFFFFFE), (67, 3, None),
                                       (2 * TILE + 1, 5, None)])
def test_every_insert_and_every_k_against_the_restatement(gpu, N, T, start):
    """One env, a few (once with ordinals that wrap), across a wave, and one
    env more than two workgroups of the table scan cover.  After every insert
    and for every k in 0..L-1 every pick of valid(k) is sampled once; the rows
    must be valid(k) in order (the compaction of the snapshot's terminals), the
    batch the restatement's, and W and P the restatement's tables."""
    rng = np.random.RandomState(1000 * N + T)
    p = Pair(N, T, STATE, gpu, start=start)
    steps = 3 * T + 1 if N <= 67 else T + 2
    sampled = 0
    for step in range(steps):
        p.add(_obs(rng, N, EX_STATE), _designed_done(step, N))
        snap = oan.dataset(p.ref)
        L = p.ref.L
        for k in range(L):
            valid = anp.valid_idxs(snap, k)
            assert len(valid) > 0 or k > 0
            if len(valid) == 0:
                continue
            B = len(valid)
            out = p.check(B, k, f'step {step} k {k}', pick=np.arange(B, dtype=np.int64))
            np.testing.assert_array_equal(_np(out['_idxs']), valid)
            P = np.concatenate([[0], np.cumsum(np.bincount(valid // L, minlength=N))])
            np.testing.assert_array_equal(_np(p.buf._atc_P), P)
            if N <= 67:
                W, P2 = oan.table(p.ref, k)
                np.testing.assert_array_equal(P2, P)
                live = np.zeros((T, N), bool)  # the slots of the env's live segments: the others are not written
                for e in range(N):
                    s0, c, _ = oan.segments(p.ref, e)
                    live[[oan._slot(s0 + i, T) for i in range(c + 1)], e] = True
                np.testing.assert_array_equal(_np(p.buf._atc_W)[live], W[live])
            if N > TILE and k == 0:  # every env holds L anchors: the running sum crosses both tile boundaries
                assert P[TILE] > 0 and P[2 * TILE] > P[TILE] and P[-1] > P[2 * TILE]
            sampled += 1
    assert sampled >= steps
    assert p.buf.atc_bad_samples() == 0


# ------------------------------------------------------------------ Philox equality
@pytest.mark.parametrize('steps', [3, 12], ids=['S<T', 'S>T'])
@pytest.mark.parametrize('k', [1, 2])
def test_philox_draws_equal_atcdataset_over_the_snapshot(gpu, k, steps):
    N, T, seed = 65, 5, 77
    ex = dict(observations=np.zeros((6, 5, 2), np.uint8))
    rng = np.random.RandomState(steps)
    p = Pair(N, T, VIS, gpu, seed=seed, ex=ex)
    p.fill(rng, steps, 0.3)
    snap = {key: v for key, v in p.buf.snapshot().items() if key != 'next_observations'}
    assert sorted(snap) == ['observations', 'terminals']
    atc = ATCDataset(Dataset(snap), VIS, seed=seed, _periodic=False)
    for call, B in enumerate((1, 64, 257)):
        assert p.buf._calls == atc._calls == call
        got = p.buf.sample_atc(B, k, record_draws=True)
        exp = atc.sample(B, k, record_draws=True)
        assert list(got) == list(exp) == ['observations', 'positive_observations', '_idxs', '_draws']
        for key in ('observations', 'positive_observations', '_idxs'):
            assert got[key].dtype == exp[key].dtype and torch.equal(got[key], exp[key]), (key, B)
        assert sorted(got['_draws']) == sorted(exp['_draws']) == ['crop_from', 'pick']
        for key in exp['_draws']:
            assert torch.equal(got['_draws'][key], exp['_draws'][key]), (key, B)
    M = len(anp.valid_idxs(oan.dataset(p.ref), k))
    assert int(p.buf._atc_P[-1]) == M >= 16 and p.buf.atc_table_builds == 1
    idxs = _np(got['_idxs'])
    # 257 uniform draws over M rows hit M (1 - (1 - 1/M)^257) >= 0.63 min(M, 257) distinct rows on average
    assert len(np.unique(idxs)) > min(M, 257) // 2
    assert tuple(got['observations'].shape) == (257, 6, 5, 6)
    assert p.buf.atc_bad_samples() == 0


# ------------------------------------------------------------ stack and crop edges
def test_stack_clamps_and_frames_are_not_shared(gpu):
    """F = 3.  An anchor at the first row of an episode with k = 1 < F - 1: the
    positive's stack clamps at the anchor.  k = 3 >= F: the two stacks share no
    frame.  Anchors in an episode whose head was overwritten and pairs across
    the physical wrap come with S > T."""
    N, T, F = 2, 8, 3
    ex = dict(observations=np.zeros((6, 5, 2), np.uint8))
    rng = np.random.RandomState(5)
    p = Pair(N, T, VIS, gpu, ex=ex)
    for step in range(11):  # live steps 3 .. 10 (slots 3 .. 7, 0, 1, 2); env 0 closes at 6, env 1 at 2 and 6
        p.add(_obs(rng, N, ex), np.array([step == 6, step in (2, 6)]))
    L, t0 = 8, 3
    # two episode starts at step 7 (slot 7: the positive lies across the wrap), an episode start at the oldest
    # live row, and the oldest live row of an episode whose head was overwritten
    first = np.array([0 * L + (7 - t0), 1 * L + (7 - t0), 1 * L + 0, 0 * L + 0], np.int64)
    for k in (1, 3):
        cf = ovn.crop_draws(rng, 4) + 1  # GCDataset's padding 3 draws 0..6; ATC's padding 4 takes 0..8
        out = p.check(4, k, f'k {k}', idxs=first, crop_from=cf)
        assert tuple(out['observations'].shape) == (4, 6, 5, 2 * F)
        # uncropped: the positive's channel blocks are rows max(o + k - 2, o) .. o + k of the same env
        plain = p.check(4, k, f'k {k} eval', idxs=first, evaluation=True)
        a, b = _np(plain['observations']), _np(plain['positive_observations'])
        obs = p.ref.cols['observations']
        for n, u in enumerate(first):
            rows = [p.ref.phys(max(u + k - (F - 1 - j), u)) for j in range(F)]
            np.testing.assert_array_equal(b[n], np.concatenate([obs[r] for r in rows], axis=-1))
            assert (a[n, ..., :2] == a[n, ..., 2:4]).all() and (a[n, ..., :2] == a[n, ..., 4:]).all()  # clamped at u
            if k == 1:
                assert (b[n, ..., :2] == b[n, ..., 2:4]).all() and (b[n, ..., :2] == a[n, ..., 4:]).all()
    valid = anp.valid_idxs(oan.dataset(p.ref), 2)
    p.check(len(valid), 2, 'every pick', pick=np.arange(len(valid)), crop_from=ovn.crop_draws(rng, len(valid)))


def test_large_frames_take_the_band_path(gpu):
    """64 x 64 x 6 uint8 at F = 3: three frames exceed the LDS budget, so the
    image is staged and composed in bands."""
    N, T, B = 4, 6, 8
    ex = dict(observations=np.zeros((64, 64, 6), np.uint8))
    rng = np.random.RandomState(6)
    p = Pair(N, T, VIS, gpu, ex=ex)
    p.fill(rng, 9, 0.25)
    valid = anp.valid_idxs(oan.dataset(p.ref), 2)
    assert len(valid) >= B
    cf = np.array([[0, 0], [8, 8], [0, 8], [8, 0], [4, 4], [3, 5], [7, 1], [1, 6]], np.int64)
    out = p.check(B, 2, 'band', pick=rng.randint(0, len(valid), B).astype(np.int64), crop_from=cf)
    assert tuple(out['observations'].shape) == (B, 64, 64, 18)
    np.testing.assert_array_equal(_np(out['_draws']['crop_from']), cf)


def test_state_buffers_and_the_other_buffer_classes(gpu):
    """frame_stack None on 2-D rows; an HGCReplayBuffer and a TRL-configured
    buffer inherit sample_atc; a stacked 2-D buffer joins on the last axis and
    draws its offsets without cropping."""
    rng = np.random.RandomState(7)
    import online_trl_np as otn

    ex3 = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))
    for cls, cfg, ex in ((GCReplayBuffer, STATE, EX_STATE), (HGCReplayBuffer, dict(STATE, subgoal_steps=3), EX_STATE),
                         (GCReplayBuffer, dict(otn.CONFIGS['geom']), ex3), (GCReplayBuffer, dict(VIS), EX_STATE)):
        p = Pair(6, 5, cfg, gpu, ex=ex, cls=cls)
        for _ in range(8):
            rows = {key: rng.randint(-99, 100, (6,) + np.array(v).shape).astype(np.array(v).dtype)
                    for key, v in ex.items()}
            p.add(rows, rng.rand(6) < 0.3)
        valid = anp.valid_idxs(oan.dataset(p.ref), 1)
        out = p.check(65, 1, cls.__name__, pick=rng.randint(0, len(valid), 65).astype(np.int64))
        F = cfg.get('frame_stack') or 1
        assert tuple(out['observations'].shape) == (65, 2 * F) and out['observations'].dtype == torch.float64
        assert ('crop_from' in out['_draws']) == (F == 3)  # the coin came up; a 2-D key is not cropped


# ---------------------------------------------------------------- caches and rebuilds
def test_table_follows_inserts_clear_and_k(gpu):
    N, T = 7, 4
    rng = np.random.RandomState(11)
    p = Pair(N, T, STATE, gpu, seed=3)
    p.fill(rng, 5, 0.3)
    assert p.buf.atc_table_builds == 0 and not hasattr(p.buf, '_atc_P')  # allocated and built by the first call
    p.buf.sample_atc(64, 1)
    assert p.buf.atc_table_builds == 1
    p.buf.sample_atc(65, 1)
    p.buf.sample_atc(1, 1, evaluation=True)
    assert p.buf.atc_table_builds == 1
    p.buf.sample_atc(64, 2)  # another k
    assert p.buf.atc_table_builds == 2
    p.buf.sample_atc(64, 1)  # and back: one table is kept
    assert p.buf.atc_table_builds == 3
    p.add(_obs(rng, N, EX_STATE), np.zeros(N, bool))
    assert p.buf.atc_table_builds == 3  # adds stayed one launch
    p.buf.sample_atc(64, 1)
    assert p.buf.atc_table_builds == 4
    p.buf.clear()
    p.ref.clear()
    p.fill(rng, 6, 0.0)
    assert p.buf.steps == 6
    out = p.buf.sample_atc(64, 1, record_draws=True)
    assert p.buf.atc_table_builds == 5
    np.testing.assert_array_equal(_np(p.buf._atc_P), oan.table(p.ref, 1)[1])
    exp, ix = oan.batch(p.ref, STATE, 1, dict(pick=_np(out['_draws']['pick'])))
    _assert_batch(out, exp, 'after clear')
    np.testing.assert_array_equal(_np(out['_idxs']), ix)


def test_out_refills_with_another_k(gpu):
    N, T = 9, 6
    rng = np.random.RandomState(12)
    a, b = Pair(N, T, STATE, gpu, seed=9), Pair(N, T, STATE, gpu, seed=9)
    for _ in range(8):
        rows, done = _obs(rng, N, EX_STATE), rng.rand(N) < 0.2
        a.add(rows, done)
        b.add(rows, done)
    first = {key: v.clone() for key, v in a.buf.sample_atc(64, 1).items()}
    second = {key: v.clone() for key, v in a.buf.sample_atc(64, 3).items()}
    out = b.buf.sample_atc(64, 1)
    ptrs = {key: v.data_ptr() for key, v in out.items()}
    assert list(out) == list(first) and all(torch.equal(out[key], first[key]) for key in first)
    again = b.buf.sample_atc(64, 3, out=out)
    assert again is out and {key: v.data_ptr() for key, v in out.items()} == ptrs
    assert all(torch.equal(out[key], second[key]) for key in second)
    assert not torch.equal(second['positive_observations'], first['positive_observations'])
    with pytest.raises(ValueError, match='64 samples'):
        b.buf.sample_atc(32, 1, out=out)
    # sample() and sample_atc() share the buffer's one counter
    assert a.buf._calls == b.buf._calls == 2
    a.buf.sample(4)
    assert a.buf._calls == 3


def test_a_buffer_that_never_draws_pairs_is_unchanged(gpu):
    rng = np.random.RandomState(2)
    a, b = Pair(5, 6, GC_CFG, gpu, seed=4), Pair(5, 6, GC_CFG, gpu, seed=4)
    for _ in range(8):
        rows, done = _obs(rng, 5, EX_STATE), rng.rand(5) < 0.3
        a.add(rows, done)
        b.add(rows, done)
    assert not any(name.startswith('_atc') or name == 'atc_table_builds' for name in vars(a.buf))
    assert a.buf.atc_table_builds == 0 and a.buf.atc_bad_samples() == 0
    assert not any(name.startswith('_atc') for name in vars(a.buf))  # asking allocates nothing either
    want = a.buf.sample(64, record_draws=True)
    b.buf.sample_atc(16, 1)
    b.buf._calls -= 1  # the call sample_atc counted
    got = b.buf.sample(64, record_draws=True)
    assert list(got) == list(want)
    for key in want:
        if key != '_draws':
            assert torch.equal(got[key], want[key]), key
    draws = {key: _np(v) for key, v in want['_draws'].items()}
    exp = a.ref.sample(GC_CFG, draws)[0]
    for key in want:  # the restatement also returns the snapshot's next_observations; this buffer stores none
        if not key.startswith('_'):
            np.testing.assert_array_equal(_np(want[key]), exp[key], err_msg=key)


# -------------------------------------------------------------------------- errors
def test_host_errors(gpu):
    p = Pair(5, 6, STATE, gpu)
    with pytest.raises(ValueError, match='empty'):
        p.buf.sample_atc(4, 1)
    with pytest.raises(ValueError, match='k must be >= 0'):
        p.buf.sample_atc(4, -1)
    rng = np.random.RandomState(0)
    p.fill(rng, 3, 0.0)
    for k in (3, 4, 100):
        with pytest.raises(ValueError) as err:
            p.buf.sample_atc(4, k)
        assert str(err.value) == f'No valid ATC indices found for k={k}.'
    assert p.buf.atc_table_builds == 0
    p.buf.sample_atc(4, 2)
    with pytest.raises(ValueError, match="unknown draw 'v_pick'"):
        p.buf.sample_atc(4, 1, draws=dict(v_pick=np.zeros(4, np.int64)))
    with pytest.raises(ValueError, match='4 entries'):
        p.buf.sample_atc(4, 1, draws=dict(pick=np.zeros(3, np.int64)))
    with pytest.raises(ValueError, match='4 entries'):
        p.buf.sample_atc(4, 1, idxs=np.zeros(5, np.int64))
    q = Pair(5, 6, dict(STATE, augment_padding=-1), gpu)
    q.fill(rng, 3, 0.0)
    with pytest.raises(ValueError, match='augment_padding'):
        q.buf.sample_atc(4, 1)
    p.buf.clear()
    with pytest.raises(ValueError, match='empty'):
        p.buf.sample_atc(4, 1)


def test_episodes_of_length_one_come_back_counted(gpu):
    """Every env done on every step: with k = 1 no segment holds a pair and the
    host cannot see it (k < live_steps).  P is all zero; the clamps keep every
    row inside the ring; every sample of the Philox path is counted, an injected
    pick raises the reference's message."""
    N, T = 5, 4
    rng = np.random.RandomState(9)
    p = Pair(N, T, VIS, gpu, ex=dict(observations=np.zeros((6, 5, 2), np.uint8)))
    p.fill(rng, 6, 1.0)
    assert oan.table(p.ref, 1)[1][-1] == 0
    total = 0
    frames = p.ref.cols['observations']
    for B in (1, 64, 257):
        out = p.buf.sample_atc(B, 1, record_draws=True)
        total += B
        assert not bool(p.buf._atc_P.any())
        idxs = _np(out['_idxs'])
        assert idxs.min() >= 0 and idxs.max() < N * T
        assert (_np(out['_draws']['pick']) == 0).all()
        # whatever row came back, its newest channel block is a frame of the ring
        got = _np(out['positive_observations'])[..., 4:6]
        cf = _np(out['_draws']['crop_from'])
        keep = (cf == 4).all(1)  # the identity crop
        assert all((frames == g).all(axis=(1, 2, 3)).any() for g in got[keep])
    torch.cuda.synchronize()
    assert p.buf.atc_bad_samples() == total
    with pytest.raises(ValueError) as err:
        p.buf.sample_atc(8, 1, draws=dict(pick=np.arange(8)))
    assert str(err.value) == 'No valid ATC indices found for k=1.'
    assert p.buf.atc_bad_samples() == total  # a checked call counts on its own
    p.check(N * T, 0, 'k = 0: every row pairs with itself', pick=np.arange(N * T), evaluation=True)


def test_explicit_bad_rows_raise_with_their_count(gpu):
    N, T = 5, 6
    rng = np.random.RandomState(8)
    p = Pair(N, T, STATE, gpu)
    p.fill(rng, 9, 0.2)
    L, k = p.ref.L, 2
    valid = anp.valid_idxs(oan.dataset(p.ref), k)
    idxs = valid[rng.randint(0, len(valid), 64)].copy()
    idxs[[3, 40, 63]] = [0 * L + L - 1, 2 * L + L - 2, N * L]  # the newest row, one before it, past the snapshot
    with pytest.raises(ValueError, match=r'\b3 of 64 samples'):
        p.buf.sample_atc(64, k, idxs=idxs)
    idxs[63] = -1
    with pytest.raises(ValueError, match=r'\b3 of 64 samples'):
        p.buf.sample_atc(64, k, idxs=idxs)
    good = valid[:10].repeat(7)[:64]
    p.check(64, k, 'still works', idxs=good)
    assert p.buf.atc_bad_samples() == 0


# ---------------------------------------------------------------- add_step end to end
def test_powderworld_pairs_through_add_step(gpu):
    n, T, steps, F, B, k = 4, 8, 12, 3, 16, 2
    env = ogbench_amd.make('powderworld-easy-v0', num_envs=n, device=gpu, max_episode_steps=5, auto_reset=True)
    obs, _ = env.reset(seed=3)
    env.step(env.sample_action())
    obs, _ = env.reset(mask=torch.tensor([True, False, True, False]))  # stagger the time limits
    shape = tuple(obs.shape[1:])
    assert shape == (32, 32, 6) and obs.dtype == torch.uint8
    ex = dict(observations=np.zeros(shape, np.uint8), actions=np.int32(0), next_observations=np.zeros(shape, np.uint8),
              terminals=np.float32(0))
    cfg = dict(GC_CFG, frame_stack=F, p_aug=1.0)
    buf = GCReplayBuffer.create(ex, n, T, cfg, device=gpu, seed=5)
    ref = onp.OnlineNp(ex, n, T)
    ends = 0
    for t in range(steps):
        prev = obs.clone()  # the env's observation view is overwritten by the step
        act = env.sample_action()
        obs, _, term, trunc, _ = env.step(act)
        term, trunc = term.clone(), trunc.clone()
        buf.add_step(prev, act, term, trunc, obs)
        ref.add_step(_np(prev), _np(act), _np(term), _np(trunc), _np(obs))
        ends += int((term | trunc).sum())
    assert ends >= n and buf.steps == steps > T
    np.testing.assert_array_equal(_np(buf['observations']), ref.cols['observations'])
    out = buf.sample_atc(B, k, record_draws=True)
    draws = {key: _np(v) for key, v in out['_draws'].items()}
    exp, ix = oan.batch(ref, cfg, k, dict(pick=draws['pick']), draws['crop_from'])
    _assert_batch(out, exp, 'powderworld')
    np.testing.assert_array_equal(_np(out['_idxs']), ix)
    snap = {key: _np(v) for key, v in buf.snapshot().items()}
    np.testing.assert_array_equal(anp.valid_idxs(snap, k), oan.pick_rows(ref, k))
    assert tuple(out['positive_observations'].shape) == (B, 32, 32, 18)
    env.close()


# ---------------------------------------------------------------------------- ABI
def test_api_version_and_einval_before_any_device_work(gpu):
    L = _online_atc.bind()
    text = open(os.path.join(ROOT, 'include', 'ogbx_online_atc.h')).read()
    assert L.ogbx_online_atc_api_version() == 1 == int(
        re.search(r'#define\s+OGBX_ONLINE_ATC_API_VERSION\s+(\d+)', text).group(1))
    N, T, B = 8, 4, 8
    i32 = dict(dtype=torch.int32, device=gpu)
    i64 = dict(dtype=torch.int64, device=gpu)
    seq, cur, end = torch.zeros((T, N), **i32), torch.zeros(N, **i32), torch.zeros((T, N), **i64)
    W = torch.full((T, N), -5, **i32)
    P = torch.full((N + 1,), -5, **i64)
    need = ctypes.c_size_t(0)
    assert L.ogbx_online_atc_table_bytes(N, ctypes.byref(need)) == _lib.OGBX_OK and need.value >= 8 * (N + 1)
    assert L.ogbx_online_atc_table_bytes(0, ctypes.byref(need)) == _lib.OGBX_EINVAL
    assert L.ogbx_online_atc_table_bytes(N, None) == _lib.OGBX_EINVAL
    tmp = torch.zeros(need.value, dtype=torch.uint8, device=gpu)
    src = torch.ones(T * N, 2, dtype=torch.float32, device=gpu)
    anchor = torch.full((B, 2), -7.0, dtype=torch.float32, device=gpu)
    positive = torch.full((B, 2), -7.0, dtype=torch.float32, device=gpu)
    host = (ctypes.c_double * (2 * B))()
    idx_out = torch.full((B,), -3, **i64)
    stream = _lib.stream_of(gpu)

    def ring(n=N, t=T, s=3, a=seq.data_ptr(), b=cur.data_ptr(), c=end.data_ptr()):
        return D.OnlineRing(n, t, s, a, b, c)

    def table(r=None, k=1, w=W.data_ptr(), p=P.data_ptr(), tp=tmp.data_ptr(), nb=None):
        return L.ogbx_online_atc_table(r if r is not None else ring(), k, w, p, tp,
                                       tmp.numel() if nb is None else nb, stream)

    bad_tables = dict(empty_ring=dict(r=ring(s=0)), n_zero=dict(r=ring(n=0)), t_zero=dict(r=ring(t=0)),
                      steps_negative=dict(r=ring(s=-1)), null_ep_seq=dict(r=ring(a=None)),
                      null_ep_end=dict(r=ring(c=None)), null_W=dict(w=None), null_P=dict(p=None),
                      null_temp=dict(tp=None), small_temp=dict(nb=need.value - 1), k_negative=dict(k=-1))
    for name, kw in bad_tables.items():
        assert table(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_atc_table' in _lib.last_error(), name

    def col(s=src.data_ptr(), a=anchor.data_ptr(), p=positive.data_ptr(), h=1, w=1, px=8, crop=0):
        return D.AtcColumn(s, a, p, h, w, px, crop)

    def outs(ix=idx_out.data_ptr(), cf=None):
        return D.AtcOutputs(ix, None, cf, None)

    def sample(r=None, k=1, w=W.data_ptr(), p=P.data_ptr(), c=col(), total=B, F=1, pad=4, idxs=None, o=outs(), draw=0):
        return L.ogbx_online_atc_sample(r if r is not None else ring(), k, w, p, c, total, F, pad, idxs, None, None,
                                        draw, 1, 0, o, stream)

    bad_samples = dict(
        empty_ring=dict(r=ring(s=0)), n_zero=dict(r=ring(n=0)), null_table=dict(r=ring(a=None)), null_W=dict(w=None),
        null_P=dict(p=None), null_col=dict(c=None), null_src=dict(c=col(s=None)), null_anchor=dict(c=col(a=None)),
        null_positive=dict(c=col(p=None)), bad_shape=dict(c=col(h=0)), total_zero=dict(total=0), k_negative=dict(k=-1),
        stack_zero=dict(F=0), stack_nine=dict(F=9), padding_negative=dict(pad=-1),
        crop_out_without_offsets=dict(o=outs(cf=idx_out.data_ptr())), row_too_wide=dict(c=col(w=70000, px=1)),
        host_output=dict(o=outs(ix=ctypes.addressof(host))), host_idxs=dict(idxs=ctypes.addressof(host)),
        host_anchor=dict(c=col(a=ctypes.addressof(host))),
    )
    for name, kw in bad_samples.items():
        assert sample(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_atc_sample' in _lib.last_error(), name

    # nothing was launched: the tables, the batch and the ring's tables are as they were
    torch.cuda.synchronize()
    assert bool((P == -5).all()) and bool((W == -5).all()) and bool((anchor == -7).all())
    assert bool((positive == -7).all()) and bool((idx_out == -3).all())
    assert bool((seq == 0).all()) and bool((end == 0).all())
    # and the same arguments, valid, do work: 3 steps, nothing done, 2 anchors per env at k = 1
    assert table() == _lib.OGBX_OK
    assert sample() == _lib.OGBX_OK
    torch.cuda.synchronize()
    assert _np(P).tolist() == [2 * e for e in range(N + 1)]
    assert bool((W[0] == 0).all()) and bool((W[1:] == -5).all())  # one live segment per env, ordinal 0
    assert bool((anchor == 1).all()) and bool((positive == 1).all())
    ix = _np(idx_out)
    assert (ix >= 0).all() and (ix < 3 * N).all() and (ix % 3 < 2).all()
