"""GPU tests of hindsight sampling over the episode ring (online_insert_kernel /
online_gc_sample_kernel via include/ogbx_online.h,
ogbench_amd.datasets.GCReplayBuffer): bit for bit against the reference's
recorded behaviour (tests/golden/online_golden.npz) and the NumPy restatement
(tests/online_np.py + oracle/gcdataset_np.py)."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ogbench_amd
import online_np as onp
from ogbench_amd import _lib
from ogbench_amd import datasets as D
from ogbench_amd.datasets import Dataset, GCDataset, GCReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_golden.npz')
PAD = 8  # margin rows on both sides of every column
SENT_F, SENT_I = -7.0, 0x5A
CFG = onp.GOLDEN_CONFIGS


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
    """A GCReplayBuffer whose columns are the middle rows of sentinel-filled
    tensors, and its restatement; the margins must keep their sentinels, the
    columns and the episode tables must equal the restatement's."""

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
        self.buf = GCReplayBuffer(cols, N, T, cfg, device=gpu, seed=seed)
        for k in cols:  # the buffer writes into the guarded storage itself
            assert self.buf[k].data_ptr() == cols[k].data_ptr()
        self.ref = onp.OnlineNp(example, N, T)
        self.rows, self.cfg, self.gpu = rows, cfg, gpu

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
        for k, (big, sent) in self.big.items():
            b = _np(big)
            assert (b[:PAD] == sent).all() and (b[PAD + self.rows:] == sent).all(), k

    def add(self, batch, done):
        self.buf.add({k: torch.as_tensor(v).to(self.gpu) for k, v in batch.items()}, torch.as_tensor(done).to(self.gpu))
        self.ref.add(batch, done)
        self.check()

    def sample(self, B, draws, cfg=None, what=''):
        """One injected-draw sample against the restatement; returns the
        restatement's (idxs, value goal idxs)."""
        cfg = self.cfg if cfg is None else cfg
        out = self.buf.sample(B, draws=draws, record_draws=True)
        exp, ix, vg, ag = self.ref.sample(cfg, draws)
        _assert_batch(out, exp, what)
        for key, v in (('_idxs', ix), ('_value_goal_idxs', vg), ('_actor_goal_idxs', ag)):
            np.testing.assert_array_equal(_np(out[key]), v, err_msg=f'{what} {key}')
        for k, v in draws.items():  # the record repeats what was injected
            np.testing.assert_array_equal(_np(out['_draws'][k]), v, err_msg=f'{what} draw {k}')
        self.check()  # a sample writes nothing into the buffer
        return ix, vg


EX2 = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))


def _example(ob):
    return dict(observations=np.zeros(ob), actions=np.zeros(2, np.float32), next_observations=np.zeros(ob))


def _rows(rng, n, ob):
    return dict(observations=rng.normal(size=(n, ob)), actions=rng.uniform(-1, 1, (n, 2)).astype(np.float32),
                next_observations=rng.normal(size=(n, ob)))


# ------------------------------------------------------------- the golden history
@pytest.mark.parametrize('cname', list(CFG))
def test_golden_history_samples_equal_the_reference(gpu, gold, cname):
    cfg = CFG[cname]
    g = Guarded(EX2, 5, 6, cfg, gpu)
    for t in range(17):
        g.add({k: gold[f'in_{k}'][t] for k in EX2}, gold['done'][t])
        S = t + 1
        if S not in (3, 6, 11, 17):
            continue
        pre = f's{S}_{cname}_'
        draws = {k[len(pre) + 5:]: v for k, v in gold.items() if k.startswith(pre + 'draw_')}
        out = g.buf.sample(64, draws=draws)
        keys = [k for k in gold[pre + 'keys'].tolist() if k != 'terminals']  # the snapshot's own column
        _assert_batch(out, {k: gold[pre + 'out_' + k] for k in keys}, pre)
        snap = g.buf.snapshot()
        assert isinstance(snap, Dataset) and sorted(snap) == sorted(list(EX2) + ['terminals'])
        for k in snap:
            got, v = _np(snap[k]), gold[f's{S}_snap_{k}']
            assert got.dtype == v.dtype and got.shape == v.shape, k
            np.testing.assert_array_equal(got, v, err_msg=f'snapshot {S} {k}')
        g.check()


# ------------------------------------------------ shapes where the kernels can go wrong
@pytest.mark.parametrize('ob', [2, 29])
@pytest.mark.parametrize('T', [1, 2, 7])
@pytest.mark.parametrize('N', [1, 5, 65, 257])
def test_every_step_against_the_restatement(gpu, N, T, ob):
    """N under, one over and across a wave and a workgroup; rows of 16 and 232
    bytes; 3 T + 1 steps of random done, so every slot is rewritten three
    times; batches of 1, 63 and 257 with random injected draws after every
    step, the geometric and the uniform config in turn."""
    rng = np.random.RandomState(1000 * N + 10 * T + ob)
    cfgs = [CFG['geom_neg'], CFG['unif_pos']]
    g = Guarded(_example(ob), N, T, cfgs[0], gpu)
    for step in range(3 * T + 1):
        g.add(_rows(rng, N, ob), rng.rand(N) < 0.3)
        cfg = cfgs[step % 2]
        g.buf.config, g.buf._cfg = cfg, D._gc_config(cfg)
        B = (1, 63, 257)[step % 3]
        g.sample(B, onp.random_draws(rng, B, g.ref.L * N), cfg, f'step {step}')


# ----------------------------------------------------------------- regime coverage
def test_the_samples_reach_every_regime(gpu):
    """The restatement alone says that these samples include a goal clipped at
    an open episode's newest row and at a closed episode's end, an idx == goal
    success, a random goal in another env and a goal whose physical row lies
    below its sample's (the ring wrapped between them); the kernel agrees on
    every one of them."""
    N, T, B = 5, 7, 257
    total = dict(clip_open=0, clip_closed=0, success=0, random_other_env=0, wrapped=0)
    for cname in ('geom_neg', 'unif_pos'):
        cfg = CFG[cname]
        rng = np.random.RandomState(7)
        g = Guarded(EX2, N, T, cfg, gpu)
        seen = dict.fromkeys(total, 0)
        for step in range(2 * T + 3):
            g.add(_rows(rng, N, 2), rng.rand(N) < 0.25)
            draws = onp.random_draws(rng, B, g.ref.L * N)
            ix, vg = g.sample(B, draws, cfg, f'{cname} step {step}')
            for k, v in onp.regimes(g.ref, ix, vg, draws, cfg).items():
                seen[k] += v
        assert all(v >= 1 for v in seen.values()), (cname, seen)
        for k in total:
            total[k] += seen[k]
    assert all(v >= 1 for v in total.values()), total


# ------------------------------------------------------------------ Philox equality
@pytest.mark.parametrize('steps', [3, 12], ids=['S<T', 'S>T'])
@pytest.mark.parametrize('cname', ['geom_neg', 'unif_pos'])
def test_philox_draws_equal_gcdataset_over_the_snapshot(gpu, cname, steps):
    N, T, seed = 65, 5, 77
    cfg = CFG[cname]
    rng = np.random.RandomState(steps)
    buf = GCReplayBuffer.create(EX2, N, T, cfg, device=gpu, seed=seed)
    for _ in range(steps):
        buf.add({k: torch.as_tensor(v).to(gpu) for k, v in _rows(rng, N, 2).items()},
                torch.as_tensor(rng.rand(N) < 0.3).to(gpu))
    gc = GCDataset(Dataset(buf.snapshot()), cfg, seed=seed)
    for call, B in enumerate((1, 64, 257)):
        assert buf._calls == gc._calls == call
        got = buf.sample(B, record_draws=True)
        exp = gc.sample(B, record_draws=True)
        for k in list(EX2) + ['value_goals', 'actor_goals', 'masks', 'rewards', '_idxs', '_value_goal_idxs',
                              '_actor_goal_idxs']:
            assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), (k, B)
        for k in exp['_draws']:
            assert torch.equal(got['_draws'][k], exp['_draws'][k]), (k, B)
    idxs = _np(got['_idxs'])
    assert idxs.min() >= 0 and idxs.max() < buf.size == min(steps, T) * N and len(np.unique(idxs)) > 100


# ---------------------------------------------------------------- add_step end to end
def test_add_step_on_a_real_auto_reset_env(gpu):
    n, T, steps = 65, 16, 40
    env = ogbench_amd.make('pointmaze-medium-v0', num_envs=n, device=gpu, auto_reset=True, max_episode_steps=7)
    obs, _ = env.reset(seed=3)
    ex = dict(observations=np.zeros(obs.shape[1:]), actions=np.zeros(2, np.float32),
              next_observations=np.zeros(obs.shape[1:]), terminals=np.float32(0))
    cfg = CFG['geom_neg']
    buf = GCReplayBuffer.create(ex, n, T, cfg, device=gpu, seed=5)
    hist = []  # the step outputs on the host
    for t in range(steps):
        prev = obs.clone()  # the env's observation view is overwritten by the step
        act = env.expert_action(seed=t)
        obs, rew, term, trunc, info = env.step(act)
        done = term | trunc
        buf.add_step(prev, act, term, trunc, obs, info['final_observation'])
        nxt = torch.where(done[:, None], info['final_observation'], obs)
        if done.any():  # the reset observation is not the episode's last
            assert not torch.equal(obs[done], info['final_observation'][done])
        hist.append(dict(observations=_np(prev), actions=_np(act).astype(np.float32), next_observations=_np(nxt),
                         terminals=_np(done).astype(np.float32), done=_np(done)))
    assert all(sum(h['done'][e] for h in hist) >= 4 for e in range(n))  # TimeLimit: every env, again and again
    snap = buf.snapshot()
    # next_observations = final_observation where done; the episodes rebuilt from the step outputs
    model = onp.Brute(n, T)
    for h in hist:
        model.add({k: h[k] for k in ex if k != 'terminals'}, h['done'])
    exp = model.snapshot({k: np.array(v).dtype for k, v in ex.items() if k != 'terminals'})
    assert sorted(snap) == sorted(ex)
    for k, v in exp.items():
        got = _np(snap[k])
        assert got.dtype == v.dtype and got.shape == v.shape, k
        np.testing.assert_array_equal(got, v, err_msg=k)
    # the buffer's own terminals column holds done as inserted
    L = T
    stored = _np(buf['terminals']).reshape(T, n)
    for t in range(steps - L, steps):
        np.testing.assert_array_equal(stored[t % T], hist[t]['terminals'])
    # every value goal lies in its sample's own episode, or was drawn as a random goal
    out = buf.sample(257, record_draws=True)
    ix, vg = _np(out['_idxs']), _np(out['_value_goal_idxs'])
    dr = {k: _np(v) for k, v in out['_draws'].items()}
    term = exp['terminals']
    ends = np.flatnonzero(term > 0)
    fin = ends[np.searchsorted(ends, ix)]
    is_cur = dr['v_u_cur'] < cfg['value_p_curgoal']
    is_traj = ~is_cur & (dr['v_u_traj'] < cfg['value_p_trajgoal'] / (1 - cfg['value_p_curgoal']))
    assert is_traj.sum() > 50 and (~is_cur & ~is_traj).sum() > 20
    assert ((vg[is_traj] > ix[is_traj]) | (ix[is_traj] == fin[is_traj])).all() and (vg[is_traj] <= fin[is_traj]).all()
    assert (vg[is_cur] == ix[is_cur]).all()
    np.testing.assert_array_equal(vg[~is_cur & ~is_traj], dr['v_pick'][~is_cur & ~is_traj])
    np.testing.assert_array_equal(_np(out['value_goals']), exp['observations'][vg])
    np.testing.assert_array_equal(_np(out['next_observations']), exp['next_observations'][ix])
    env.close()


# -------------------------------------------------------------------------- errors
def test_errors_and_clear(gpu):
    cfg = CFG['geom_neg']
    t = lambda a: torch.as_tensor(a).to(gpu)  # noqa: E731
    for name in ('masks', 'rewards', 'value_goals', 'actor_goals', 'valids'):
        with pytest.raises(ValueError, match=name):
            GCReplayBuffer.create(dict(EX2, **{name: 0.0}), 5, 6, cfg, device=gpu)
    with pytest.raises(AssertionError):
        GCReplayBuffer.create(EX2, 5, 6, dict(cfg, value_p_curgoal=0.5), device=gpu)
    g = Guarded(EX2, 5, 6, cfg, gpu)
    with pytest.raises(ValueError, match='empty'):
        g.buf.sample(4)
    rng = np.random.RandomState(0)
    rows = {k: t(v) for k, v in _rows(rng, 5, 2).items()}
    done = torch.zeros(5, dtype=torch.bool, device=gpu)
    with pytest.raises(ValueError, match='shape'):  # a wrong N
        g.buf.add({k: t(v) for k, v in _rows(rng, 4, 2).items()}, done[:4])
    with pytest.raises(ValueError, match='5 entries'):
        g.buf.add(rows, done[:4])
    with pytest.raises(ValueError, match='keys'):  # a missing and an extra key
        g.buf.add({k: v for k, v in rows.items() if k != 'actions'}, done)
    with pytest.raises(ValueError, match='keys'):
        g.buf.add(dict(rows, extra=rows['actions']), done)
    with pytest.raises(ValueError, match='keys'):  # add_step needs the step layout
        g.buf.add_step(rows['observations'], rows['actions'], done, done, rows['next_observations'])
    g.check()  # refused on the host: nothing moved
    assert g.buf.steps == 0
    for _ in range(8):
        g.add(_rows(rng, 5, 2), rng.rand(5) < 0.5)
    assert g.buf.steps == 8 and g.buf.live_steps == 6 and int(g.buf.cur_seq.sum()) > 0
    old = g.buf['actions']
    g.buf['actions'] = torch.zeros(31, 2, device=gpu)  # a column of another length
    with pytest.raises(ValueError, match='replaced'):
        g.buf.add(rows, done)
    with pytest.raises(ValueError, match='replaced'):
        g.buf.sample(4)
    g.buf['actions'] = old
    g.buf.clear()
    g.ref.clear()
    assert g.buf.steps == 0 and g.buf.live_steps == 0 and _np(g.buf.cur_seq).tolist() == [0] * 5
    with pytest.raises(ValueError, match='empty'):
        g.buf.sample(4)
    g.add(_rows(rng, 5, 2), np.array([True, False, False, True, False]))  # starts at step 0 again
    assert g.buf.steps == 1 and _np(g.buf.cur_seq).tolist() == [1, 0, 0, 1, 0]
    g.sample(63, onp.random_draws(rng, 63, 5))


def test_out_refills_in_place(gpu):
    cfg = CFG['unif_pos']
    rng = np.random.RandomState(4)
    bufs = [GCReplayBuffer.create(EX2, 65, 4, cfg, device=gpu, seed=9) for _ in range(2)]
    for _ in range(6):
        rows, done = _rows(rng, 65, 2), rng.rand(65) < 0.3
        for b in bufs:
            b.add({k: torch.as_tensor(v).to(gpu) for k, v in rows.items()}, torch.as_tensor(done).to(gpu))
    a, b = bufs
    first = {k: v.clone() for k, v in a.sample(64).items()}
    second = {k: v.clone() for k, v in a.sample(64).items()}
    assert not torch.equal(first['observations'], second['observations'])
    out = b.sample(64)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    assert all(torch.equal(out[k], first[k]) for k in first)
    again = b.sample(64, out=out)
    assert again is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
    assert all(torch.equal(out[k], second[k]) for k in second)
    with pytest.raises(ValueError, match='64 samples'):  # another batch size
        b.sample(32, out=out)
    # a refill after further inserts draws from the rows held then
    rows, done = _rows(rng, 65, 2), rng.rand(65) < 0.3
    for x in bufs:
        x.add({k: torch.as_tensor(v).to(gpu) for k, v in rows.items()}, torch.as_tensor(done).to(gpu))
    a._calls = b._calls
    want = a.sample(64)
    assert b.sample(64, out=out) is out and all(torch.equal(out[k], want[k]) for k in want)


# ---------------------------------------------------------------------------- ABI
def test_api_version_and_einval_before_any_device_work(gpu):
    L = D._bind()
    text = open(os.path.join(ROOT, 'include', 'ogbx_online.h')).read()
    assert L.ogbx_online_api_version() == int(re.search(r'#define\s+OGBX_ONLINE_API_VERSION\s+(\d+)', text).group(1))
    N, T = 8, 4
    cfg = D._gc_config(CFG['geom_neg'])
    seq = torch.full((T, N), 3, dtype=torch.int32, device=gpu)
    cur = torch.full((N,), 3, dtype=torch.int32, device=gpu)
    end = torch.full((T, N), 3, dtype=torch.int64, device=gpu)
    dst = torch.full((T * N, 2), SENT_F, dtype=torch.float32, device=gpu)
    src = torch.ones(N, 2, dtype=torch.float32, device=gpu)
    done = torch.ones(N, dtype=torch.uint8, device=gpu)
    out = torch.full((N, 2), SENT_F, dtype=torch.float32, device=gpu)
    masks = torch.full((N,), SENT_F, dtype=torch.float64, device=gpu)
    rewards = torch.full((N,), SENT_F, dtype=torch.float64, device=gpu)
    stream = _lib.stream_of(gpu)

    def ring(n=N, t=T, s=5, a=seq.data_ptr(), b=cur.data_ptr(), c=end.data_ptr()):
        return D.OnlineRing(n, t, s, a, b, c)

    def col(dst_p=dst.data_ptr(), src_p=src.data_ptr(), alt=None, elems=2, sdt=4, ddt=4, op=0):
        return D.ReplayInsertColumn(dst_p, src_p, alt, elems, sdt, ddt, op, 0)

    def insert(r=None, cols=(col(),), ncols=None, dn=done.data_ptr(), sel=None):
        arr = (D.ReplayInsertColumn * max(len(cols), 1))(*cols) if cols is not None else None
        return L.ogbx_online_insert(r if r is not None else ring(), arr, len(cols) if ncols is None else ncols, dn, sel,
                                    stream)

    bad_inserts = dict(
        n_zero=dict(r=ring(n=0)), t_zero=dict(r=ring(t=0)), n_huge=dict(r=ring(n=1 << 31)),
        rows_huge=dict(r=ring(n=(1 << 31) - 1, t=(1 << 31) - 1)), steps_negative=dict(r=ring(s=-1)),
        null_ep_seq=dict(r=ring(a=None)), null_cur_seq=dict(r=ring(b=None)), null_ep_end=dict(r=ring(c=None)),
        null_done=dict(dn=None), null_cols=dict(cols=None, ncols=1), too_many_columns=dict(cols=(col(),) * 17),
        negative_columns=dict(ncols=-1), null_dst=dict(cols=(col(dst_p=None),)), null_src=dict(cols=(col(src_p=None),)),
        row_elems_zero=dict(cols=(col(elems=0),)), row_over_4_mib=dict(cols=(col(elems=(1 << 19) + 1),)),
        src_dtype=dict(cols=(col(sdt=6),)), dst_dtype_bool=dict(cols=(col(ddt=0),)), op=dict(cols=(col(op=2),)),
        alt_without_select=dict(cols=(col(alt=src.data_ptr()),)),
    )
    for name, kw in bad_inserts.items():
        assert insert(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_insert' in _lib.last_error(), name

    def gcol(src_p=dst.data_ptr(), dst_p=out.data_ptr(), rb=8, select=0, stride=0):
        return D.GcColumn(src_p, dst_p, rb, select, stride)

    def sample(r=None, cols=(gcol(),), ncols=None, total=N, m=masks.data_ptr(), rw=rewards.data_ptr(), cf=cfg):
        arr = (D.GcColumn * max(len(cols), 1))(*cols) if cols is not None else None
        batch = D.OnlineBatch(ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None,
                              len(cols) if ncols is None else ncols, 0, total, None, None, None, m, rw)
        return L.ogbx_online_gc_sample(r if r is not None else ring(), cf, batch, None, None, 1, 0, stream)

    bad_samples = dict(
        empty_ring=dict(r=ring(s=0)), n_zero=dict(r=ring(n=0)), null_table=dict(r=ring(a=None)), null_cfg=dict(cf=None),
        total_zero=dict(total=0), null_masks=dict(m=None), null_rewards=dict(rw=None), null_cols=dict(cols=None, ncols=1),
        too_many_columns=dict(cols=(gcol(),) * 17), null_src=dict(cols=(gcol(src_p=None),)),
        null_dst=dict(cols=(gcol(dst_p=None),)), row_bytes=dict(cols=(gcol(rb=0),)),
        select_next=dict(cols=(gcol(select=1),)), select=dict(cols=(gcol(select=4),)), stride=dict(cols=(gcol(stride=4),)),
    )
    for name, kw in bad_samples.items():
        assert sample(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_online_gc_sample' in _lib.last_error(), name
    assert L.ogbx_online_clear(ring(n=0), stream) == _lib.OGBX_EINVAL

    # nothing was launched: tables, column and batch are as they were
    torch.cuda.synchronize()
    assert bool((seq == 3).all()) and bool((cur == 3).all()) and bool((end == 3).all())
    assert bool((dst == SENT_F).all()) and bool((out == SENT_F).all()) and bool((masks == SENT_F).all())
    # and the same arguments, valid, do work: step 5 goes to slot 1, closing episode 3 of every env
    assert insert() == _lib.OGBX_OK
    assert sample(r=ring(s=6)) == _lib.OGBX_OK
    torch.cuda.synchronize()
    assert bool((dst[N:2 * N] == 1).all()) and bool((dst[:N] == SENT_F).all()) and bool((dst[2 * N:] == SENT_F).all())
    assert _np(cur).tolist() == [4] * N and _np(end[3 % T]).tolist() == [5] * N and _np(seq[1]).tolist() == [3] * N
    assert bool(((out == 1) | (out == SENT_F)).all()) and bool(((masks == 0) | (masks == 1)).all())
