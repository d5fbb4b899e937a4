"""GPU tests of hierarchical hindsight sampling over the episode ring
(online_hgc_sample_kernel via include/ogbx_online_hgc.h,
ogbench_amd.datasets.HGCReplayBuffer): bit for bit against the reference's
recorded behaviour (tests/golden/online_hgc_golden.npz) and the NumPy
restatement (tests/online_hgc_np.py: oracle/gcdataset_np.hgc_sample over the
snapshot of tests/online_np.OnlineNp)."""

import os
import re

import numpy as np
import pytest
import torch

import ogbench_amd
import online_hgc_np as ohn
import online_np as onp
from ogbench_amd import _lib
from ogbench_amd import datasets as D
from ogbench_amd.datasets import Dataset, HGCDataset, HGCReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_hgc_golden.npz')
PAD = 8  # margin rows on both sides of every column
SENT_F, SENT_I = -7.0, 0x5A
CFG = ohn.GOLDEN_CONFIGS
IDX_KEYS = (('_idxs', 'idxs'), ('_high_value_goal_idxs', 'hvg'), ('_high_actor_goal_idxs', 'hag'),
            ('_low_value_goal_idxs', 'lvg'))


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


class Guarded:
    """An HGCReplayBuffer whose columns are the middle rows of sentinel-filled
    tensors, and its restatement; the margins must keep their sentinels, and
    the columns, the episode tables and the step tables must be what the
    restatement holds: a sample writes nothing into the buffer."""

    def __init__(self, example, N, T, cfg, gpu, seed=1):
        self.big, cols = {}, {}
        rows = N * T
        for k, v in example.items():
            v = np.array(v)
            sent = SENT_F if v.dtype.kind == 'f' else SENT_I
            big = torch.full((rows + 2 * PAD,) + v.shape, sent, dtype=torch.from_numpy(np.zeros(0, v.dtype)).dtype,
                             device=gpu)
            big[PAD:PAD + rows] = 0
            self.big[k] = (big, sent)
            cols[k] = big[PAD:PAD + rows]
        self.buf = HGCReplayBuffer(cols, N, T, cfg, device=gpu, seed=seed)
        for k in cols:  # the buffer writes into the guarded storage itself
            assert self.buf[k].data_ptr() == cols[k].data_ptr()
        self.ref = onp.OnlineNp(example, N, T)
        self.rows, self.cfg, self.gpu = rows, cfg, gpu
        self.tables = [_np(t).copy() for t in self.buf._hv_tab + self.buf._lv_tab]
        assert [len(t) for t in self.tables] == [self.buf.value_subgoal_steps + 1] * 2 + \
            [self.buf.low_subgoal_steps + 1] * 2

    def check(self):
        buf, ref = self.buf, self.ref
        assert (buf.steps, buf.live_steps) == (ref.S, ref.L)
        for k, v in ref.cols.items():
            got = _np(buf[k])
            assert got.dtype == v.dtype and got.shape == v.shape, k
            np.testing.assert_array_equal(got, v, err_msg=k)
        for name in ('ep_seq', 'cur_seq', 'ep_end'):
            got, v = _np(getattr(buf, name)), getattr(ref, name)
            assert got.dtype == v.dtype and got.shape == v.shape, name
            np.testing.assert_array_equal(got, v, err_msg=name)
        for t, v in zip(buf._hv_tab + buf._lv_tab, self.tables):
            np.testing.assert_array_equal(_np(t), v)
        self.margins()

    def margins(self):
        for k, (big, sent) in self.big.items():
            b = _np(big)
            assert (b[:PAD] == sent).all() and (b[PAD + self.rows:] == sent).all(), k

    def add(self, batch, done):
        self.buf.add({k: torch.as_tensor(v).to(self.gpu) for k, v in batch.items()}, torch.as_tensor(done).to(self.gpu))
        self.ref.add(batch, done)
        self.check()

    def sample(self, B, draws, what=''):
        """One injected-draw sample against the restatement; returns the
        restatement's (batch, indices)."""
        out = self.buf.sample(B, draws=draws, record_draws=True)
        exp, ix = ohn.hgc_sample(self.ref, self.cfg, draws)
        _assert_batch(out, exp, what)
        for key, name in IDX_KEYS:
            got = _np(out[key])
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got, ix[name], err_msg=f'{what} {key}')
        assert sorted(out['_draws']) == sorted(self.buf._draw_keys)
        for k, v in draws.items():  # the record repeats what was injected
            np.testing.assert_array_equal(_np(out['_draws'][k]), v, err_msg=f'{what} draw {k}')
        self.check()
        return exp, ix


EX2 = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))


def _example(ob):
    return dict(observations=np.zeros(ob), actions=np.zeros(2, np.float32), next_observations=np.zeros(ob))


def _rows(rng, n, ob):
    return dict(observations=rng.normal(size=(n, ob)), actions=rng.uniform(-1, 1, (n, 2)).astype(np.float32),
                next_observations=rng.normal(size=(n, ob)))


def _low(cfg):
    return cfg.get('low_discount') is not None


# ------------------------------------------------------------- the golden history
@pytest.mark.parametrize('cname', list(CFG))
def test_golden_history_samples_equal_the_reference(gpu, gold, cname):
    cfg = CFG[cname]
    g = Guarded(EX2, ohn.N, ohn.T, cfg, gpu)
    for t in range(ohn.STEPS):
        g.add({k: gold[f'in_{k}'][t] for k in EX2}, gold['done'][t])
        S = t + 1
        if S not in ohn.SNAPS:
            continue
        pre = f's{S}_{cname}_'
        draws = {k[len(pre) + 5:]: v for k, v in gold.items() if k.startswith(pre + 'draw_')}
        out = g.buf.sample(ohn.B, draws=draws)
        keys = [k for k in gold[pre + 'keys'].tolist() if k != 'terminals']  # the snapshot's own column
        assert len(keys) == (26 if _low(cfg) else 25)
        _assert_batch(out, {k: gold[pre + 'out_' + k] for k in keys}, pre)
        g.check()


# ------------------------------------------------ shapes where the kernel can go wrong
@pytest.mark.parametrize('ob', [2, 29])
@pytest.mark.parametrize('T', [1, 2, 7])
@pytest.mark.parametrize('N', [1, 5, 65, 257])
def test_every_step_against_the_restatement(gpu, N, T, ob):
    """N under, one over and across a wave and a workgroup; rows of 16 and 232
    bytes (the 4-byte flat copy and the general one); 3 T + 1 steps of random
    done, so every slot is rewritten three times; batches of 1, 63 and 257 with
    random injected draws after every step, one buffer for ``hiql`` and one
    for ``hlow`` (with the l_* draws).  T = 1: every step count is 0 and every
    selector the sample's own row."""
    rng = np.random.RandomState(1000 * N + 10 * T + ob)
    gs = [Guarded(_example(ob), N, T, CFG[c], gpu) for c in ('hiql', 'hlow')]
    for step in range(3 * T + 1):
        rows, done = _rows(rng, N, ob), rng.rand(N) < 0.3
        B = (1, 63, 257)[step % 3]
        for g in gs:
            g.add(rows, done)
            exp, ix = g.sample(B, ohn.random_draws(rng, B, g.ref.L * N, _low(g.cfg)), f'step {step}')
            if T == 1:
                assert not exp['high_value_subgoal_steps'].any() and not exp['low_value_subgoal_steps'].any()
                np.testing.assert_array_equal(exp['low_actor_goal_observations'], exp['observations'])


# ----------------------------------------------------------------- regime coverage
def test_the_samples_reach_every_regime(gpu):
    """The restatement alone says that these samples include a full subgoal
    step, a step clipped at an open episode's newest row, at a closed episode's
    end and by the goal, a goal behind the sample, a random goal in another
    env, a subgoal whose physical row lies below its sample's (the ring wrapped
    between them) and a low value goal equal to idx; the kernel agrees on every
    one of them (``Guarded.sample`` compares the whole batch)."""
    N, T, B = 5, 7, 257
    for cname in ('hiql', 'hlow'):
        cfg = CFG[cname]
        rng = np.random.RandomState(7)
        g = Guarded(EX2, N, T, cfg, gpu)
        seen = {}
        for step in range(2 * T + 3):
            g.add(_rows(rng, N, 2), rng.rand(N) < 0.25)
            draws = ohn.random_draws(rng, B, g.ref.L * N, _low(cfg), max_geom=4)
            exp, ix = g.sample(B, draws, f'{cname} step {step}')
            for k, v in ohn.gpu_regimes(g.ref, ix, draws, cfg, exp['high_value_subgoal_steps']).items():
                seen[k] = seen.get(k, 0) + v
        if not _low(cfg):
            assert seen.pop('low_goal_is_idx') < 0
        assert all(v >= 1 for v in seen.values()), (cname, seen)


# --------------------------------------------------------- out-of-range injections
@pytest.mark.parametrize('cname', ['hiql', 'hlow'])
def test_out_of_range_injections_stay_in_bounds(gpu, cname):
    """Designed inputs, safe by the kernel's clamps: picks of -5 and L N + 5,
    geometric draws of 10^6, and the ep_end entries of closed episodes
    overwritten with -1 and 2^40.  The call returns, every index output lies in
    [0, L N), every step output in [0, K], and the margins are intact."""
    cfg = CFG[cname]
    N, T, B = 5, 7, 257
    rng = np.random.RandomState(11)
    g = Guarded(EX2, N, T, cfg, gpu)
    for _ in range(2 * T + 2):
        g.add(_rows(rng, N, 2), rng.rand(N) < 0.3)
    npick = g.ref.L * N
    draws = ohn.random_draws(rng, B, npick, _low(cfg))
    for k in [k for k in draws if k.endswith('pick')]:
        draws[k][0::3] = -5
        draws[k][1::3] = npick + 5
    for k in [k for k in draws if k.endswith('geom')]:
        draws[k][0::2] = 10 ** 6
    saved = g.buf.ep_end.clone()
    assert int(g.buf.cur_seq.sum()) > 0  # there are closed episodes
    bad = torch.where(torch.arange(T * N, device=gpu).reshape(T, N) % 2 == 0, -1, 1 << 40).to(torch.int64)
    for tables in (bad, saved):
        g.buf.ep_end.copy_(tables)
        for kw in (dict(draws=draws), dict(draws={k: v for k, v in draws.items() if k != 'pick'},
                                           idxs=draws['pick'])):
            out = g.buf.sample(B, record_draws=True, **kw)
            torch.cuda.synchronize()
            for key, _ in IDX_KEYS:
                v = _np(out[key])
                assert v.min() >= 0 and v.max() < npick, key
            for key, K in (('high_value_subgoal_steps', g.buf.value_subgoal_steps),
                           ('low_value_subgoal_steps', g.buf.low_subgoal_steps)):
                v = _np(out[key])
                assert v.min() >= 0 and v.max() <= K, key
            # every row came from the ring: no sentinel reached the batch
            for key in ('observations', 'high_value_goals', 'high_actor_next_observations',
                        'low_actor_goal_observations', 'low_actor_next_observations'):
                assert not bool((out[key] == SENT_F).any()), key
            g.margins()
    g.check()  # the tables are restored and nothing else moved
    # with its own tables the clamped call is the restatement's under the clamped picks
    clamped = {k: (np.clip(v, 0, npick - 1) if k.endswith('pick') else v) for k, v in draws.items()}
    exp, ix = ohn.hgc_sample(g.ref, cfg, clamped)
    _assert_batch(out, exp, 'clamped')


# ------------------------------------------------------------------ Philox equality
@pytest.mark.parametrize('steps', [3, 12], ids=['S<T', 'S>T'])
@pytest.mark.parametrize('cname', ['hiql', 'hlow'])
def test_philox_draws_equal_hgcdataset_over_the_snapshot(gpu, cname, steps):
    N, T, seed = 65, 5, 77
    cfg = CFG[cname]
    rng = np.random.RandomState(steps)
    buf = HGCReplayBuffer.create(EX2, N, T, cfg, device=gpu, seed=seed)
    for _ in range(steps):
        buf.add({k: torch.as_tensor(v).to(gpu) for k, v in _rows(rng, N, 2).items()},
                torch.as_tensor(rng.rand(N) < 0.3).to(gpu))
    hgc = HGCDataset(Dataset(buf.snapshot()), cfg, seed=seed)
    for call, B in enumerate((1, 64, 257)):
        assert buf._calls == hgc._calls == call
        got = buf.sample(B, record_draws=True)
        exp = hgc.sample(B, record_draws=True)
        common = [k for k in exp if k != '_draws' and k != 'terminals']
        assert [k for k in got if k != '_draws'] == common
        for k in common:
            assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), (k, B)
        assert sorted(got['_draws']) == sorted(exp['_draws'])
        assert ('l_pick' in got['_draws']) == _low(cfg)
        for k in exp['_draws']:
            assert torch.equal(got['_draws'][k], exp['_draws'][k]), (k, B)
    idxs = _np(got['_idxs'])
    assert idxs.min() >= 0 and idxs.max() < buf.size == min(steps, T) * N and len(np.unique(idxs)) > 100


# ---------------------------------------------------------------- add_step end to end
def test_add_step_on_a_real_auto_reset_env(gpu):
    n, T, steps, B = 8, 16, 40, 257
    env = ogbench_amd.make('pointmaze-medium-v0', num_envs=n, device=gpu, auto_reset=True, max_episode_steps=7)
    obs, _ = env.reset(seed=3)
    ex = dict(observations=np.zeros(obs.shape[1:]), actions=np.zeros(2, np.float32),
              next_observations=np.zeros(obs.shape[1:]), terminals=np.float32(0))
    cfg = CFG['hiql']
    buf = HGCReplayBuffer.create(ex, n, T, cfg, device=gpu, seed=5)
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
    assert closed >= 4 * n and buf.steps == steps > T  # TimeLimit: every env, again and again
    for k, v in ref.cols.items():
        np.testing.assert_array_equal(_np(buf[k]), v, err_msg=k)
    rng = np.random.RandomState(2)
    draws = ohn.random_draws(rng, B, T * n, False)
    out = buf.sample(B, draws=draws)
    exp, ix = ohn.hgc_sample(ref, cfg, draws)
    assert list(exp)[:4] == list(ex)  # the buffer's own terminals: done as inserted
    _assert_batch(out, exp, 'add_step')
    assert exp['high_value_subgoal_steps'].max() == 3 and (exp['terminals'] > 0).any()
    env.close()


# ------------------------------------------------------------------- smaller checks
def _filled(gpu, cfg, example=EX2, N=65, T=4, steps=6, seed=9, copies=1, rows=None):
    rng = np.random.RandomState(4)
    bufs = [HGCReplayBuffer.create(example, N, T, cfg, device=gpu, seed=seed) for _ in range(copies)]
    for _ in range(steps):
        r, done = (rows or (lambda: _rows(rng, N, 2)))(), rng.rand(N) < 0.3
        for b in bufs:
            b.add({k: torch.as_tensor(v).to(gpu) for k, v in r.items()}, torch.as_tensor(done).to(gpu))
    return bufs, rng


@pytest.mark.parametrize('cname', ['hiql', 'hlow'])
def test_out_refills_in_place_and_aliases_hold(gpu, cname):
    cfg = CFG[cname]
    (a, b), rng = _filled(gpu, cfg, copies=2)
    first = {k: v.clone() for k, v in a.sample(64).items()}
    second = {k: v.clone() for k, v in a.sample(64).items()}
    assert not torch.equal(first['observations'], second['observations'])
    out = b.sample(64)
    assert out['high_value_reps'] is out['observations'] and out['value_goals'] is out['high_value_goals']
    assert out['high_actor_targets'] is out['high_actor_actions']
    assert ('low_value_goals' in out) == _low(cfg) and len(out) == (26 if _low(cfg) else 25)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    assert all(torch.equal(out[k], first[k]) for k in first)
    again = b.sample(64, out=out)
    assert again is out and {k: v.data_ptr() for k, v in out.items()} == ptrs and b._calls == 2
    assert all(torch.equal(out[k], second[k]) for k in second)
    with pytest.raises(ValueError, match='64 samples'):  # another batch size
        b.sample(32, out=out)
    # a refill after a further insert draws from the rows held then
    rows, done = _rows(rng, 65, 2), rng.rand(65) < 0.3
    for x in (a, b):
        x.add({k: torch.as_tensor(v).to(gpu) for k, v in rows.items()}, torch.as_tensor(done).to(gpu))
    a._calls = b._calls
    want = a.sample(64)
    assert b.sample(64, out=out) is out and all(torch.equal(out[k], want[k]) for k in want)
    # the parent's helpers go through this sample
    sub = b.get_subset(torch.arange(10, device=gpu))
    assert 'low_actor_next_observations' in sub and len(sub['masks']) == 10
    ri = b.get_random_idxs(33)
    assert ri.dtype == torch.int64 and len(ri) == 33 and int(ri.min()) >= 0 and int(ri.max()) < b.size


def test_oracle_reps_are_the_goal_source(gpu):
    ex = dict(EX2, oracle_reps=np.zeros(3, np.float32))
    cfg = CFG['hlow']
    N, T = 5, 7
    rng = np.random.RandomState(5)
    g = Guarded(ex, N, T, cfg, gpu)
    for step in range(T + 3):
        g.add(dict(_rows(rng, N, 2), oracle_reps=rng.normal(size=(N, 3)).astype(np.float32)), rng.rand(N) < 0.3)
    exp, ix = g.sample(63, ohn.random_draws(rng, 63, g.ref.L * N, True))
    for k in ('high_value_goals', 'high_value_actions', 'low_value_goals', 'high_actor_goals', 'high_actor_actions',
              'low_actor_goals'):
        assert exp[k].shape == (63, 3) and exp[k].dtype == np.float32, k
    assert exp['low_actor_goal_observations'].shape == (63, 2) and 'oracle_reps' in exp


def test_value_errors(gpu):
    cfg = CFG['hlow']
    for name in ('masks', 'actor_goals', 'high_value_reps', 'low_value_goals', 'high_actor_targets',
                 'low_actor_next_observations'):
        with pytest.raises(ValueError, match=name):
            HGCReplayBuffer.create(dict(EX2, **{name: 0.0}), 5, 6, cfg, device=gpu)
    with pytest.raises(KeyError):  # the hierarchical config is needed
        HGCReplayBuffer.create(EX2, 5, 6, onp.GOLDEN_CONFIGS['geom_neg'], device=gpu)
    with pytest.raises(ValueError, match='subgoal'):
        HGCReplayBuffer.create(EX2, 5, 6, dict(cfg, low_subgoal_steps=0), device=gpu)
    buf = HGCReplayBuffer.create(EX2, 5, 6, cfg, device=gpu)
    with pytest.raises(ValueError, match='empty'):
        buf.sample(4)
    (buf,), rng = _filled(gpu, cfg, N=5, T=6, steps=8)
    with pytest.raises(ValueError, match='unknown draw'):
        buf.sample(4, draws=dict(x_pick=np.zeros(4, np.int64)))
    with pytest.raises(ValueError, match='4 entries'):
        buf.sample(4, draws=dict(l_geom=np.ones(5, np.int64)))
    with pytest.raises(ValueError, match='4 entries'):
        buf.sample(4, idxs=np.zeros(3, np.int64))
    (plain,), _ = _filled(gpu, CFG['hiql'], N=5, T=6, steps=8)
    with pytest.raises(ValueError, match='unknown draw'):  # no low value goals, no l_* draws
        plain.sample(4, draws=dict(l_geom=np.ones(4, np.int64)))
    old = buf['actions']
    buf['actions'] = torch.zeros(31, 2, device=gpu)  # a column of another length
    with pytest.raises(ValueError, match='replaced'):
        buf.sample(4)
    buf['actions'] = old
    assert len(buf.sample(4)['masks']) == 4


# ---------------------------------------------------------------------------- ABI
def test_api_version_and_einval_before_any_device_work(gpu):
    L = D._bind()
    text = open(os.path.join(ROOT, 'include', 'ogbx_online_hgc.h')).read()
    assert L.ogbx_online_hgc_api_version() == int(
        re.search(r'#define\s+OGBX_ONLINE_HGC_API_VERSION\s+(\d+)', text).group(1))
    N, T = 8, 4
    cfg = D._gc_config(CFG['hlow'])
    seq = torch.full((T, N), 3, dtype=torch.int32, device=gpu)
    cur = torch.full((N,), 3, dtype=torch.int32, device=gpu)
    end = torch.full((T, N), 3, dtype=torch.int64, device=gpu)
    src = torch.ones(T * N, 2, dtype=torch.float32, device=gpu)
    out = torch.full((N, 2), SENT_F, dtype=torch.float32, device=gpu)
    sc_i = [torch.full((N,), SENT_I, dtype=torch.int64, device=gpu) for _ in range(3)]
    sc_f = [torch.full((N,), SENT_F, dtype=torch.float64, device=gpu) for _ in range(6)]
    tabs = D._subgoal_tables(0.97, 4, False, gpu) + D._subgoal_tables(0.97, 1, False, gpu)
    stream = _lib.stream_of(gpu)

    def ring(n=N, t=T, s=5, a=seq.data_ptr(), b=cur.data_ptr(), c=end.data_ptr()):
        return D.OnlineRing(n, t, s, a, b, c)

    def hcfg(v=4, lo=1, a=2, has_low=1, ld=0.95, tables=None):
        tables = [t.data_ptr() for t in tabs] if tables is None else tables
        return D.HgcConfig(v, lo, a, has_low, 0, ld, *tables)

    def outs(drop=None):
        p = dict(high_value_offsets=sc_i[0], high_value_subgoal_steps=sc_i[1], high_value_masks=sc_f[0],
                 high_value_rewards=sc_f[1], low_value_subgoal_steps=sc_i[2], low_value_masks=sc_f[2],
                 low_value_rewards=sc_f[3], masks=sc_f[4], rewards=sc_f[5])
        return D.HgcOutputs(None, None, None, None, *[None if k == drop else t.data_ptr() for k, t in p.items()])

    def gcol(src_p=src.data_ptr(), dst_p=out.data_ptr(), rb=8, select=0, stride=0):
        return D.GcColumn(src_p, dst_p, rb, select, stride)

    def sample(r=None, cf=cfg, hc=None, cols=(gcol(),), ncols=None, total=N, o=None):
        arr = (D.GcColumn * max(len(cols), 1))(*cols) if cols is not None else None
        return L.ogbx_online_hgc_sample(r if r is not None else ring(), cf, hc if hc is not None else hcfg(), arr,
                                        len(cols) if ncols is None else ncols, total, None,
                                        o if o is not None else outs(), None, 1, 0, stream)

    three = [t.data_ptr() for t in tabs[:3]]
    bad = dict(
        empty_ring=dict(r=ring(s=0)), n_zero=dict(r=ring(n=0)), t_zero=dict(r=ring(t=0)), n_huge=dict(r=ring(n=1 << 31)),
        rows_huge=dict(r=ring(n=(1 << 31) - 1, t=(1 << 31) - 1)), steps_negative=dict(r=ring(s=-1)),
        null_ep_seq=dict(r=ring(a=None)), null_cur_seq=dict(r=ring(b=None)), null_ep_end=dict(r=ring(c=None)),
        null_cfg=dict(cf=None), total_zero=dict(total=0), null_cols=dict(cols=None, ncols=1),
        too_many_columns=dict(cols=(gcol(),) * 33), negative_columns=dict(ncols=-1),
        null_src=dict(cols=(gcol(src_p=None),)), null_dst=dict(cols=(gcol(dst_p=None),)),
        row_bytes=dict(cols=(gcol(rb=0),)), select_next=dict(cols=(gcol(select=1),)),
        select_ten=dict(cols=(gcol(select=10),)), select_negative=dict(cols=(gcol(select=-1),)),
        stride=dict(cols=(gcol(stride=4),)), value_steps_zero=dict(hc=hcfg(v=0)), low_steps_zero=dict(hc=hcfg(lo=0)),
        actor_steps_negative=dict(hc=hcfg(a=-1)), low_discount_one=dict(hc=hcfg(ld=1.0)),
        null_table=dict(hc=hcfg(tables=three + [None])), null_first_table=dict(hc=hcfg(tables=[None] + three)),
        **{f'missing_{k}': dict(o=outs(drop=k)) for k in D._HGC_SCALARS[4:]},
    )
    for name, kw in bad.items():
        assert sample(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_hgc_sample' in _lib.last_error(), name
    assert L.ogbx_online_hgc_sample(None, cfg, hcfg(), None, 0, N, None, outs(), None, 1, 0, stream) == _lib.OGBX_EINVAL
    assert L.ogbx_online_hgc_sample(ring(), cfg, None, None, 0, N, None, outs(), None, 1, 0, stream) == _lib.OGBX_EINVAL
    assert L.ogbx_online_hgc_sample(ring(), cfg, hcfg(), None, 0, N, None, None, None, 1, 0, stream) == _lib.OGBX_EINVAL

    # nothing was launched: tables and batch are as they were
    torch.cuda.synchronize()
    assert bool((seq == 3).all()) and bool((cur == 3).all()) and bool((end == 3).all())
    assert bool((out == SENT_F).all()) and all(bool((t == SENT_I).all()) for t in sc_i)
    assert all(bool((t == SENT_F).all()) for t in sc_f)
    # and the same arguments, valid, do work -- every selector, 32 columns: all rows are open episodes of ones
    assert sample() == _lib.OGBX_OK
    wide = torch.full((32, N, 2), SENT_F, dtype=torch.float32, device=gpu)
    sels = [0, 2, 3, 4, 5, 6, 7, 8, 9]
    cols32 = tuple(gcol(dst_p=wide[i].data_ptr(), select=sels[i % len(sels)]) for i in range(32))
    assert sample(cols=cols32) == _lib.OGBX_OK
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and bool((wide == 1).all())
    assert bool(((sc_i[1] >= 0) & (sc_i[1] <= 4)).all()) and bool(((sc_i[2] >= 0) & (sc_i[2] <= 1)).all())
    assert bool(((sc_f[4] == 0) | (sc_f[4] == 1)).all())
