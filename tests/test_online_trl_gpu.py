"""GPU tests of TRL batches over the episode ring (ogbx_online_trl_table /
online_trl_sample_kernel via include/ogbx_online_trl.h, a
ogbench_amd.datasets.GCReplayBuffer whose config has a TRL agent name): bit for
bit against the reference's recorded behaviour
(tests/golden/online_trl_golden.npz), the NumPy restatement
(tests/online_trl_np.py) and the offline TRL sampler over the snapshot."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ogbench_amd
import online_np as onp
import online_trl_np as otn
import trl_np as tnp
from ogbench_amd import _lib, _online_trl
from ogbench_amd import datasets as D
from ogbench_amd.datasets import Dataset, GCDataset, GCReplayBuffer, HGCReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_trl_golden.npz')
CFG = otn.CONFIGS
EX2 = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))
TILE = _online_trl.ONLINE_TRL_TABLE_TILE
IDX_KEYS = (('_idxs', 'idxs'), ('_value_goal_idxs', 'vg'), ('_actor_goal_idxs', 'ag'), ('_value_midpoint_idxs', 'mid'))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _np(t):
    return t.cpu().numpy()


def _assert_batch(out, exp, what=''):
    assert [k for k in out if not k.startswith('_')] == list(exp), what
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (what, k, got.dtype, got.shape, v.dtype, v.shape)
        np.testing.assert_array_equal(got, v, err_msg=f'{what} {k}')


def _assert_aliases(out, reps=False):
    assert out['actor_goal_observations'] is out['value_goal_observations']
    assert out['value_offsets'].dtype == torch.int64 and out['value_midpoint_offsets'].dtype == torch.int64
    if not reps:
        assert out['value_goal_observations'] is out['value_goals']
        assert out['value_midpoint_goals'] is out['value_midpoint_observations']
        assert out['value_cur_goals'] is out['observations']
    else:
        assert out['value_cur_goals'] is out['oracle_reps']
        assert out['value_goals'] is not out['value_goal_observations']
    assert out['value_next_goals'] is not out['next_observations']


def _rows(rng, n, ex=EX2):
    out = {}
    for k, v in ex.items():
        v = np.array(v)
        out[k] = rng.randint(-99, 100, (n,) + v.shape).astype(v.dtype)
    return out


class Pair:
    """A TRL GCReplayBuffer and its restatement, fed the same rows."""

    def __init__(self, N, T, cfg, gpu, seed=1, ex=EX2):
        self.buf = GCReplayBuffer.create(ex, N, T, cfg, device=gpu, seed=seed)
        self.ref = onp.OnlineNp(ex, N, T)
        self.cfg, self.gpu, self.ex = cfg, gpu, ex

    def add(self, batch, done):
        self.buf.add({k: torch.as_tensor(v).to(self.gpu) for k, v in batch.items()}, torch.as_tensor(done).to(self.gpu))
        self.ref.add(batch, done)

    def clear(self):
        self.buf.clear()
        self.ref.clear()

    def check_table(self):
        """P as the last sample built it."""
        P = _np(self.buf._trl_P)
        exp = otn.table(self.ref)
        assert P.dtype == exp.dtype and P.shape == exp.shape
        np.testing.assert_array_equal(P, exp)

    def injected(self, B, draws, what='', idxs=None):
        out = self.buf.sample(B, draws=draws, idxs=idxs, record_draws=True)
        exp, ix = otn.batch(self.ref, self.cfg, draws, idxs=idxs)
        _assert_batch(out, exp, what)
        for key, name in IDX_KEYS:
            np.testing.assert_array_equal(_np(out[key]), ix[name], err_msg=f'{what} {key}')
        for k, v in draws.items():  # the record repeats what was injected
            if idxs is None or k != 'pick':
                np.testing.assert_array_equal(_np(out['_draws'][k]), v, err_msg=f'{what} draw {k}')
        self.check_table()
        return out, ix

    def philox(self, B, what='', **kw):
        """A Philox call replayed through the restatement from its record."""
        out = self.buf.sample(B, record_draws=True, **kw)
        draws = {k: _np(v) for k, v in out['_draws'].items()}
        exp, ix = otn.batch(self.ref, self.cfg, draws)
        _assert_batch(out, exp, what)
        for key, name in IDX_KEYS:
            np.testing.assert_array_equal(_np(out[key]), ix[name], err_msg=f'{what} {key}')
        assert (ix['idxs'] <= ix['mid']).all() and (ix['mid'] < ix['vg']).all()
        table = otn.table(self.ref)[-1]
        assert draws['pick'].min() >= 0 and draws['pick'].max() < table
        self.check_table()
        return out, ix


# ------------------------------------------------------------- the golden history
@pytest.mark.parametrize('cname', list(CFG))
def test_golden_history_samples_equal_the_reference(gpu, gold, cname):
    cfg = CFG[cname]
    p = Pair(5, 6, cfg, gpu)
    assert gold['snap_steps'].tolist() == [2, 3, 6, 11, 17]
    for t in range(17):
        p.add({k: gold[f'hist_{k}'][t] for k in EX2}, gold['done'][t])
        S = t + 1
        if S not in (2, 3, 6, 11, 17):
            continue
        _, draws, exp, keys = tnp.fixture_case(gold, f's{S}_{cname}')
        out = p.buf.sample(64, draws=draws)
        keys = [k for k in keys if k != 'terminals']  # the snapshot's own column
        _assert_batch(out, {k: exp[k] for k in keys}, f's{S}_{cname}')
        _assert_aliases(out)
        p.check_table()
        assert int(p.buf._trl_P[-1]) == int(gold[f's{S}_pickable'])
    assert p.buf.trl_table_builds == 5


# ------------------------------------------------ shapes where the kernels can go wrong
@pytest.mark.parametrize('N,T', [(1, 2), (3, 4), (67, 3), (2 * TILE + 1, 5)])
def test_every_step_against_the_restatement(gpu, N, T):
    """One env, a few, across a wave, and one env more than two workgroups of
    the table scan cover (its running sum crosses two workgroup boundaries);
    3 T + 1 steps of random done, so every slot is rewritten three times;
    batches of 1, 64, 65 and 257 (a full tile, one spilled over, a partial one)
    with random injected draws after every step that leaves a pickable row, the
    geometric and the uniform config in turn."""
    rng = np.random.RandomState(1000 * N + T)
    cfgs = [CFG['geom'], CFG['unif']]
    p = Pair(N, T, cfgs[0], gpu)
    sampled = 0
    for step in range(3 * T + 1):
        p.add(_rows(rng, N), rng.rand(N) < 0.3)
        if p.ref.S < 2 or otn.table(p.ref)[-1] == 0:
            continue
        cfg = cfgs[step % 2]
        p.cfg, p.buf.config, p.buf._cfg = cfg, cfg, D._gc_config(cfg)
        B = (1, 64, 65, 257)[sampled % 4]
        p.injected(B, otn.random_draws(rng, B, p.ref, cfg), f'step {step}')
        sampled += 1
    assert sampled >= (4 if N > 1 else 1)  # one env: only while its older row is not done
    if N > TILE:
        P = _np(p.buf._trl_P)
        assert P[TILE] > 0 and P[2 * TILE] > P[TILE] and P[-1] > P[2 * TILE]


# ------------------------------------------------------------------ Philox equality
@pytest.mark.parametrize('steps', [3, 12], ids=['S<T', 'S>T'])
@pytest.mark.parametrize('cname', list(CFG))
def test_philox_draws_equal_gcdataset_over_the_snapshot(gpu, cname, steps):
    N, T, seed = 65, 5, 77
    cfg = CFG[cname]
    rng = np.random.RandomState(steps)
    buf = GCReplayBuffer.create(EX2, N, T, cfg, device=gpu, seed=seed)
    for _ in range(steps):
        buf.add({k: torch.as_tensor(v).to(gpu) for k, v in _rows(rng, N).items()},
                torch.as_tensor(rng.rand(N) < 0.3).to(gpu))
    gc = GCDataset(Dataset(buf.snapshot()), cfg, seed=seed)
    assert gc._trl and buf._trl
    for call, B in enumerate((1, 64, 257)):
        assert buf._calls == gc._calls == call
        got = buf.sample(B, record_draws=True)
        exp = gc.sample(B, record_draws=True)
        pub = [k for k in exp if not k.startswith('_') and k != 'terminals']
        assert [k for k in got if not k.startswith('_')] == pub
        for k in pub + ['_idxs', '_value_goal_idxs', '_actor_goal_idxs', '_value_midpoint_idxs']:
            assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), (k, B)
        assert sorted(got['_draws']) == sorted(exp['_draws'])
        for k in exp['_draws']:
            assert torch.equal(got['_draws'][k], exp['_draws'][k]), (k, B)
    M = gc._valid.numel()
    assert int(buf._trl_P[-1]) == M > 64 and buf.trl_table_builds == 1
    idxs = _np(got['_idxs'])
    assert idxs.min() >= 0 and idxs.max() < buf.size == min(steps, T) * N
    # 257 uniform draws over M rows hit M (1 - (1 - 1/M)^257) >= 0.63 min(M, 257) distinct rows on average
    assert len(np.unique(idxs)) > min(M, 257) // 2
    assert buf.trl_bad_samples() == 0


# ------------------------------------------------------------------ table upkeep
def test_table_follows_inserts_and_clear(gpu):
    """sample, insert, sample, clear(), re-insert other episodes up to the same
    ``steps``, sample: each equals the restatement; samples at one step build
    the table once."""
    N, T = 7, 4
    rng = np.random.RandomState(11)
    p = Pair(N, T, CFG['geom'], gpu, seed=3)
    for _ in range(5):
        p.add(_rows(rng, N), rng.rand(N) < 0.3)
    assert p.buf.trl_table_builds == 0  # built lazily, by sample
    p.philox(64, 'first')
    assert p.buf.trl_table_builds == 1
    p.philox(65, 'same step')
    p.philox(1, 'same step')
    assert p.buf.trl_table_builds == 1
    p.add(_rows(rng, N), np.ones(N, bool))
    before = otn.table(p.ref)
    p.philox(64, 'after an insert')
    assert p.buf.trl_table_builds == 2
    p.clear()
    for _ in range(6):
        p.add(_rows(rng, N), np.zeros(N, bool))
    assert p.buf.steps == 6 and not np.array_equal(otn.table(p.ref), before)
    p.philox(64, 'after clear and as many steps')
    assert p.buf.trl_table_builds == 3
    # adds stayed one launch: nothing of the table moved without a sample
    p.add(_rows(rng, N), rng.rand(N) < 0.5)
    assert p.buf.trl_table_builds == 3


def test_a_buffer_without_a_trl_agent_name_is_unchanged(gpu):
    rng = np.random.RandomState(2)
    for cfg in (onp.GOLDEN_CONFIGS['geom_neg'], dict(onp.GOLDEN_CONFIGS['geom_neg'], agent_name='crl')):
        buf = GCReplayBuffer.create(EX2, 5, 6, cfg, device=gpu, seed=4)
        ref = onp.OnlineNp(EX2, 5, 6)
        for _ in range(8):
            rows, done = _rows(rng, 5), rng.rand(5) < 0.3
            buf.add({k: torch.as_tensor(v).to(gpu) for k, v in rows.items()}, torch.as_tensor(done).to(gpu))
            ref.add(rows, done)
        # the class's own sample: no table, no counter, nothing bound on the instance
        assert 'sample' not in vars(buf) and not buf._trl
        assert not hasattr(buf, '_trl_P') and not hasattr(buf, 'trl_table_builds')
        out = buf.sample(64, record_draws=True)
        draws = {k: _np(v) for k, v in out['_draws'].items()}
        exp = ref.sample(cfg, draws)[0]
        _assert_batch(out, exp)
        assert list(exp) == list(EX2) + ['value_goals', 'actor_goals', 'masks', 'rewards']


# ----------------------------------------------------------------- arguments
def test_out_idxs_and_evaluation(gpu):
    N, T = 65, 4
    rng = np.random.RandomState(4)
    a, b = Pair(N, T, CFG['unif'], gpu, seed=9), Pair(N, T, CFG['unif'], gpu, seed=9)
    for _ in range(6):
        rows, done = _rows(rng, N), rng.rand(N) < 0.3
        a.add(rows, done)
        b.add(rows, done)
    first = {k: v.clone() for k, v in a.buf.sample(64).items()}
    second = {k: v.clone() for k, v in a.buf.sample(64, evaluation=True).items()}
    assert not torch.equal(first['value_midpoint_observations'], second['value_midpoint_observations'])
    out = b.buf.sample(64)
    _assert_aliases(out)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    assert list(out) == list(first) and all(torch.equal(out[k], first[k]) for k in first)
    again = b.buf.sample(64, out=out)
    assert again is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
    assert all(torch.equal(out[k], second[k]) for k in second)
    with pytest.raises(ValueError, match='64 samples'):
        b.buf.sample(32, out=out)
    # a refill after a further insert draws from the table of that step
    rows, done = _rows(rng, N), rng.rand(N) < 0.3
    a.add(rows, done)
    b.add(rows, done)
    want = a.buf.sample(64)
    assert b.buf.sample(64, out=out) is out and all(torch.equal(out[k], want[k]) for k in want)
    assert a.buf.trl_table_builds == b.buf.trl_table_builds == 2
    # explicit flat rows, any pickable ones in any order
    rows_ = otn.pick_rows(b.ref)
    idxs = rows_[rng.randint(0, len(rows_), 65)]
    draws = otn.random_draws(rng, 65, b.ref, b.cfg)
    _, ix = otn.batch(b.ref, b.cfg, draws, idxs=idxs)
    draws['midpoint'] = ix['idxs'] + (rng.rand(65) * (ix['vg'] - ix['idxs'])).astype(np.int64)
    got, ix = b.injected(65, draws, 'explicit idxs', idxs=idxs)
    np.testing.assert_array_equal(_np(got['_idxs']), idxs)
    assert (_np(got['_draws']['pick']) == -1).all()


def test_oracle_reps_and_a_terminals_column(gpu):
    ex = dict(observations=np.zeros(3, np.float32), actions=np.zeros(2, np.float32),
              next_observations=np.zeros(3, np.float32), terminals=np.float32(0), oracle_reps=np.zeros(2, np.float32))
    rng = np.random.RandomState(6)
    p = Pair(6, 5, CFG['geom'], gpu, seed=2, ex=ex)
    for _ in range(8):
        done = rng.rand(6) < 0.3
        p.add(dict(_rows(rng, 6, ex), terminals=done.astype(np.float32)), done)
    out, _ = p.philox(65, 'reps')
    _assert_aliases(out, reps=True)
    assert out['value_goals'].shape == (65, 2) and out['value_goal_observations'].shape == (65, 3)


# -------------------------------------------------------------------------- errors
def test_construction_and_sample_errors(gpu):
    cfg = CFG['geom']
    with pytest.raises(ValueError, match='value_p_randomgoal'):
        GCReplayBuffer.create(EX2, 5, 6, dict(cfg, value_p_trajgoal=0.5, value_p_randomgoal=0.5), device=gpu)
    with pytest.raises(ValueError, match='value_p_curgoal'):
        GCReplayBuffer.create(EX2, 5, 6, dict(cfg, value_p_trajgoal=0.5, value_p_curgoal=0.5), device=gpu)
    with pytest.raises(ValueError, match='actions'):
        GCReplayBuffer.create(dict(observations=np.zeros(2)), 5, 6, cfg, device=gpu)
    with pytest.raises(ValueError, match='next_actions'):
        GCReplayBuffer.create(dict(EX2, next_actions=np.zeros(2, np.float32)), 5, 6, cfg, device=gpu)
    with pytest.raises(NotImplementedError, match='frame_stack'):
        GCReplayBuffer.create(EX2, 5, 6, dict(cfg, frame_stack=2), device=gpu)
    with pytest.raises(NotImplementedError, match='p_aug'):
        GCReplayBuffer.create(EX2, 5, 6, dict(cfg, p_aug=0.5), device=gpu)
    assert GCReplayBuffer.create(EX2, 5, 6, dict(cfg, p_aug=0.0), device=gpu)._trl  # not a live p_aug
    for name in D.TRL_AGENTS:
        with pytest.raises(NotImplementedError, match='HGCReplayBuffer'):
            HGCReplayBuffer.create(EX2, 5, 6, dict(cfg, agent_name=name, subgoal_steps=3), device=gpu)
        assert GCReplayBuffer.create(EX2, 5, 6, dict(cfg, agent_name=name), device=gpu)._trl
    p = Pair(5, 6, cfg, gpu)
    with pytest.raises(ValueError, match='empty'):
        p.buf.sample(4)
    rng = np.random.RandomState(0)
    p.add(_rows(rng, 5), np.zeros(5, bool))
    with pytest.raises(ValueError, match='steps >= 2'):
        p.buf.sample(4)
    assert p.buf.trl_table_builds == 0
    p.add(_rows(rng, 5), np.zeros(5, bool))
    p.philox(4)
    with pytest.raises(ValueError, match='unknown draw'):
        p.buf.sample(4, draws=dict(l_pick=np.zeros(4, np.int64)))
    with pytest.raises(ValueError, match='4 entries'):
        p.buf.sample(4, draws=dict(midpoint=np.zeros(3, np.int64)))
    p.clear()
    with pytest.raises(ValueError, match='empty'):
        p.buf.sample(4)


def test_explicit_newest_rows_raise_with_their_count(gpu):
    N, T = 5, 6
    rng = np.random.RandomState(8)
    p = Pair(N, T, CFG['geom'], gpu)
    for _ in range(9):
        p.add(_rows(rng, N), rng.rand(N) < 0.2)
    L = p.ref.L
    rows = otn.pick_rows(p.ref)
    idxs = rows[rng.randint(0, len(rows), 64)].copy()
    idxs[[3, 40, 63]] = [0 * L + L - 1, 2 * L + L - 1, N * L - 1]  # newest rows, the snapshot's last among them
    with pytest.raises(ValueError, match=r'\b3 of 64 samples'):
        p.buf.sample(64, idxs=idxs)
    out = p.buf.sample(64, idxs=rows[:10].repeat(7)[:64], record_draws=True)  # still works
    np.testing.assert_array_equal(_np(out['_idxs']), rows[:10].repeat(7)[:64])
    # an injected value goal at the sample itself is counted too
    draws = {k: _np(v) for k, v in out['_draws'].items() if k != 'pick'}
    draws['v_geom'] = draws['v_geom'].copy()
    draws['v_geom'][:2] = 0
    with pytest.raises(ValueError, match=r'\b2 of 64 samples'):
        p.buf.sample(64, idxs=rows[:10].repeat(7)[:64], draws=draws)
    assert p.buf.trl_bad_samples() == 0  # checked calls count on their own


def test_every_row_done_comes_back_counted(gpu):
    """Every env done on every step: no row can be picked, P is all zero.  The
    clamps keep every index inside the ring; every sample is counted."""
    N, T = 5, 4
    rng = np.random.RandomState(9)
    p = Pair(N, T, CFG['unif'], gpu)
    for _ in range(6):
        p.add(_rows(rng, N), np.ones(N, bool))
    assert otn.table(p.ref)[-1] == 0
    total = 0
    for B in (1, 64, 257):
        out = p.buf.sample(B, record_draws=True)
        total += B
        p.check_table()
        for key in ('_idxs', '_value_goal_idxs', '_actor_goal_idxs', '_value_midpoint_idxs'):
            v = _np(out[key])
            assert v.min() >= 0 and v.max() < N * T, key
        np.testing.assert_array_equal(_np(out['_value_midpoint_idxs']), _np(out['_idxs']))
        snap = p.ref.snapshot()
        np.testing.assert_array_equal(_np(out['observations']), snap['observations'][_np(out['_idxs'])])
    torch.cuda.synchronize()
    assert p.buf.trl_bad_samples() == total


# ------------------------------------- the host path shared with the dataset samplers
def _tiny_sampler(kind, gpu, seed=1):
    """A dataset sampler of one family and mode over 3 trajectories of 10 rows."""
    rng = np.random.RandomState(4)
    visual, R = kind.endswith('visual'), 30
    term = np.zeros(R, np.float32)
    term[9::10] = 1
    obs = rng.randint(0, 256, (R, 8, 8, 3)).astype(np.uint8) if visual else rng.normal(size=(R, 2))
    data = dict(observations=obs, actions=rng.normal(size=(R, 2)).astype(np.float32), terminals=term, valids=1 - term)
    cfg = dict(CFG['geom'], p_aug=0.5 if visual else None, frame_stack=3 if visual else None)
    if not kind.startswith('gc_trl'):
        cfg.pop('agent_name')
    if kind.startswith('hgc'):
        return D.HGCDataset(Dataset(data, device=gpu), dict(cfg, subgoal_steps=3), seed=seed)
    return GCDataset(Dataset(data, device=gpu), cfg, seed=seed)


@pytest.mark.parametrize('kind', ['gc', 'gc_visual', 'gc_trl', 'hgc', 'hgc_visual'])
def test_dataset_samplers_name_a_wrong_length(gpu, kind):
    s = _tiny_sampler(kind, gpu)
    assert s._trl == (kind == 'gc_trl') and s._visual == kind.endswith('visual')
    with pytest.raises(ValueError, match=r'idxs must have 8 entries, got 7'):
        s.sample(8, idxs=np.arange(7))
    with pytest.raises(ValueError, match=r"draw 'v_geom' must have 8 entries, got 9"):
        s.sample(8, draws=dict(v_geom=np.ones(9, np.int64)))
    out = s.sample(8, idxs=np.arange(8), record_draws=True)  # still works
    np.testing.assert_array_equal(_np(out['_idxs']), np.arange(8))


@pytest.mark.parametrize('kind', ['gc', 'hgc'])
def test_unknown_draws_are_skipped_by_datasets_and_refused_by_rings(gpu, kind):
    """The dataset samplers skip a draw they do not take (the reference's
    fixtures hand HGCDataset an 'l_dist'); the ring buffers raise."""
    a, b = _tiny_sampler(kind, gpu, seed=6), _tiny_sampler(kind, gpu, seed=6)
    got = a.sample(8, draws=dict(l_dist=np.zeros(8), x_pick=np.zeros(3, np.int64)), record_draws=True)
    exp = b.sample(8, record_draws=True)
    assert list(got) == list(exp) and list(got['_draws']) == list(exp['_draws'])
    for k, v in exp.items():
        for kk, t in (v.items() if k == '_draws' else [(k, v)]):
            assert torch.equal(got[k][kk] if k == '_draws' else got[k], t), (k, kk)
    cls, cfg = (HGCReplayBuffer, dict(otn.CONFIGS['geom'], subgoal_steps=3)) if kind == 'hgc' else \
        (GCReplayBuffer, dict(otn.CONFIGS['geom']))
    cfg.pop('agent_name')
    buf = cls.create(EX2, 3, 6, cfg, device=gpu, seed=6)
    buf.add({k: torch.as_tensor(v).to(gpu) for k, v in _rows(np.random.RandomState(0), 3).items()},
            torch.zeros(3, dtype=torch.bool, device=gpu))
    with pytest.raises(ValueError, match="unknown draw 'l_dist'"):
        buf.sample(8, draws=dict(l_dist=np.zeros(8)))


def test_trl_layout_is_one_for_dataset_and_ring(gpu):
    """A TRL GCDataset and a TRL GCReplayBuffer over the same snapshot return
    the same keys, in the same order, after the data's own."""
    cfg, rng = CFG['geom'], np.random.RandomState(2)
    buf = GCReplayBuffer.create(EX2, 3, 6, cfg, device=gpu, seed=1)
    for t in range(5):
        buf.add({k: torch.as_tensor(v).to(gpu) for k, v in _rows(rng, 3).items()},
                torch.as_tensor(np.arange(3) == t).to(gpu))
    gc = GCDataset(Dataset(buf.snapshot()), cfg, seed=1)
    got, exp = buf.sample(8), gc.sample(8)
    layout = [k for k, _, _ in D._TRL_LAYOUT]
    assert list(got)[:len(buf)] == list(buf) and list(exp)[:len(gc.dataset)] == list(gc.dataset)
    assert list(got)[len(buf):] == list(exp)[len(gc.dataset):] == layout
    assert sorted(layout[:4]) == sorted(GCReplayBuffer.RESERVED[:4]) and layout[4:] == list(GCReplayBuffer._TRL_KEYS)
    for k in layout:
        assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), k
    _assert_aliases(got)
    _assert_aliases(exp)


# ---------------------------------------------------------------- add_step end to end
def test_add_step_on_a_real_auto_reset_env(gpu):
    n, T, steps = 64, 8, 20
    env = ogbench_amd.make('pointmaze-medium-v0', num_envs=n, device=gpu, auto_reset=True, max_episode_steps=5)
    obs, _ = env.reset(seed=3)
    ex = dict(observations=np.zeros(obs.shape[1:]), actions=np.zeros(2, np.float32),
              next_observations=np.zeros(obs.shape[1:]), terminals=np.float32(0))
    cfg = CFG['geom']
    buf = GCReplayBuffer.create(ex, n, T, cfg, device=gpu, seed=5)
    ref = onp.OnlineNp(ex, n, T)
    closed = 0
    for t in range(steps):
        prev = obs.clone()  # the env's observation view is overwritten by the step
        act = env.expert_action(seed=t)
        obs, rew, term, trunc, info = env.step(act)
        buf.add_step(prev, act, term, trunc, obs, info['final_observation'])
        ref.add_step(_np(prev), _np(act).astype(np.float32), _np(term), _np(trunc), _np(obs),
                     _np(info['final_observation']))
        closed += int((term | trunc).sum())
        if t >= 1:
            out = buf.sample(65, record_draws=True)
            draws = {k: _np(v) for k, v in out['_draws'].items()}
            exp, ix = otn.batch(ref, cfg, draws)
            _assert_batch(out, exp, f'step {t}')
            np.testing.assert_array_equal(_np(out['_value_midpoint_idxs']), ix['mid'])
            np.testing.assert_array_equal(_np(buf._trl_P), otn.table(ref))
    assert closed >= 3 * n and buf.trl_table_builds == steps - 1 and buf.trl_bad_samples() == 0
    env.close()


# ---------------------------------------------------------------------------- ABI
def test_api_version_and_einval_before_any_device_work(gpu):
    L = _online_trl.bind()
    text = open(os.path.join(ROOT, 'include', 'ogbx_online_trl.h')).read()
    assert L.ogbx_online_trl_api_version() == 1 == int(
        re.search(r'#define\s+OGBX_ONLINE_TRL_API_VERSION\s+(\d+)', text).group(1))
    N, T, B = 8, 4, 8
    SENT = -7.0
    cfg = D._gc_config(CFG['geom'])
    i32 = dict(dtype=torch.int32, device=gpu)
    i64 = dict(dtype=torch.int64, device=gpu)
    seq, cur, end = torch.zeros((T, N), **i32), torch.zeros(N, **i32), torch.zeros((T, N), **i64)
    P = torch.full((N + 1,), -5, **i64)
    need = ctypes.c_size_t(0)
    assert L.ogbx_online_trl_table_bytes(N, ctypes.byref(need)) == _lib.OGBX_OK and need.value >= 1
    assert L.ogbx_online_trl_table_bytes(0, ctypes.byref(need)) == _lib.OGBX_EINVAL
    assert L.ogbx_online_trl_table_bytes(N, None) == _lib.OGBX_EINVAL
    tmp = torch.zeros(need.value, dtype=torch.uint8, device=gpu)
    src = torch.ones(T * N, 2, dtype=torch.float32, device=gpu)
    dst = torch.full((B, 2), SENT, dtype=torch.float32, device=gpu)
    masks = torch.full((B,), SENT, dtype=torch.float64, device=gpu)
    rewards = torch.full((B,), SENT, dtype=torch.float64, device=gpu)
    host = (ctypes.c_double * B)()
    rec_one = torch.zeros(B, **i64)
    stream = _lib.stream_of(gpu)

    def ring(n=N, t=T, s=3, a=seq.data_ptr(), b=cur.data_ptr(), c=end.data_ptr()):
        return D.OnlineRing(n, t, s, a, b, c)

    def table(r=None, p=P.data_ptr(), tp=tmp.data_ptr(), nb=None):
        return L.ogbx_online_trl_table(r if r is not None else ring(), p, tp, tmp.numel() if nb is None else nb, stream)

    bad_tables = dict(empty_ring=dict(r=ring(s=0)), n_zero=dict(r=ring(n=0)), t_zero=dict(r=ring(t=0)),
                      steps_negative=dict(r=ring(s=-1)), null_ep_seq=dict(r=ring(a=None)), null_P=dict(p=None),
                      null_temp=dict(tp=None), small_temp=dict(nb=need.value - 1))
    for name, kw in bad_tables.items():
        assert table(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_trl_table' in _lib.last_error(), name

    def gcol(src_p=src.data_ptr(), dst_p=dst.data_ptr(), rb=8, select=0, stride=0):
        return D.GcColumn(src_p, dst_p, rb, select, stride)

    def outs(m=masks.data_ptr(), rw=rewards.data_ptr()):
        return D.TrlOutputs(None, None, None, None, None, None, m, rw, None)

    def sample(r=None, p=P.data_ptr(), cf=cfg, cols=(gcol(),), ncols=None, total=B, o=outs(), rec=None, mid=None):
        arr = (D.GcColumn * max(len(cols), 1))(*cols) if cols is not None else None
        return L.ogbx_online_trl_sample(r if r is not None else ring(), p, cf, arr,
                                        len(cols) if ncols is None else ncols, total, None, mid, 1, 0, o, rec, None,
                                        stream)

    cur_cfg = D._gc_config(dict(CFG['geom'], value_p_curgoal=0.5, value_p_trajgoal=0.5))
    rand_cfg = D._gc_config(dict(CFG['geom'], value_p_randomgoal=0.5, value_p_trajgoal=0.5))
    part_rec = D.GcDrawRecord(rec_one.data_ptr(), *[None] * 10)
    bad_samples = dict(
        empty_ring=dict(r=ring(s=0)), n_zero=dict(r=ring(n=0)), null_table=dict(r=ring(a=None)), null_P=dict(p=None),
        null_cfg=dict(cf=None), null_out=dict(o=None), total_zero=dict(total=0), null_cols=dict(cols=None, ncols=1),
        too_many_columns=dict(cols=(gcol(),) * 33), null_src=dict(cols=(gcol(src_p=None),)),
        null_dst=dict(cols=(gcol(dst_p=None),)), row_bytes=dict(cols=(gcol(rb=0),)),
        select=dict(cols=(gcol(select=5),)), stride=dict(cols=(gcol(stride=4),)), value_cur=dict(cf=cur_cfg),
        value_random=dict(cf=rand_cfg), incomplete_record=dict(rec=part_rec),
        host_pointer=dict(o=outs(rw=ctypes.addressof(host))),
    )
    for name, kw in bad_samples.items():
        assert sample(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_trl_sample' in _lib.last_error(), name

    # nothing was launched: the table, the batch and the ring's tables are as they were
    torch.cuda.synchronize()
    assert bool((P == -5).all()) and bool((dst == SENT).all()) and bool((masks == SENT).all())
    assert bool((seq == 0).all()) and bool((end == 0).all())
    # and the same arguments, valid, do work: 3 steps, nothing done, 2 pickable rows per env
    assert table() == _lib.OGBX_OK
    cols = tuple(gcol(select=s) for s in range(5))
    assert sample(cols=cols) == _lib.OGBX_OK
    torch.cuda.synchronize()
    assert _np(P).tolist() == [2 * e for e in range(N + 1)]
    assert bool((dst == 1).all()) and bool((masks == 1).all()) and bool((rewards == 0).all())
