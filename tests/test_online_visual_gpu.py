"""GPU tests of visual batches over the episode ring
(online_visual_gather_kernel via include/ogbx_online_visual.h;
``GCReplayBuffer`` / ``HGCReplayBuffer`` with ``frame_stack`` / ``p_aug``): bit
for bit against the batches put together from the reference's own code
(tests/golden/online_visual_golden.npz), the NumPy restatement
(tests/online_visual_np.py) and the offline visual samplers over the
snapshot."""

import os

import numpy as np
import pytest
import torch

import ogbench_amd
import online_hgc_np as ohn
import online_np as onp
import online_visual_np as ovn
from ogbench_amd.datasets import Dataset, GCDataset, GCReplayBuffer, HGCReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_visual_golden.npz')
PAD = 8  # margin rows on both sides of every column
SENT_F, SENT_I = -7.0, 0x5A
GC_CFG = ovn.GOLDEN_CONFIGS['geom']
HGC_CFG = ovn.GOLDEN_CONFIGS['hlow']


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _np(t):
    return t.cpu().numpy()


def _dev(batch, gpu):
    return {k: torch.as_tensor(v).to(gpu) for k, v in batch.items()}


def _assert_batch(out, exp, what=''):
    assert [k for k in out if not k.startswith('_')] == list(exp), what
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (what, k, got.dtype, got.shape, v.dtype, v.shape)
        np.testing.assert_array_equal(got, v, err_msg=f'{what} {k}')


class Guarded:
    """A visual ring buffer whose columns are the middle rows of
    sentinel-filled tensors, and its restatement (as test_online_gpu.Guarded):
    the margins must keep their sentinels, the columns and the episode tables
    must equal the restatement's, and the ring holds unstacked frames."""

    def __init__(self, example, N, T, cfg, gpu, hgc=False, seed=1):
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
        self.buf = (HGCReplayBuffer if hgc else GCReplayBuffer)(cols, N, T, cfg, device=gpu, seed=seed)
        for k in cols:  # the buffer reads the guarded storage itself
            assert self.buf[k].data_ptr() == cols[k].data_ptr()
        self.ref = onp.OnlineNp(example, N, T)
        self.rows, self.cfg, self.gpu, self.hgc = rows, cfg, gpu, hgc

    def check(self):
        buf, ref = self.buf, self.ref
        assert (buf.steps, buf.live_steps) == (ref.S, ref.L)
        for k, v in ref.cols.items():
            got = _np(buf[k])
            assert got.dtype == v.dtype and got.shape == v.shape, k  # unstacked
            np.testing.assert_array_equal(got, v, err_msg=k)
        for name in ('ep_seq', 'cur_seq', 'ep_end'):
            np.testing.assert_array_equal(_np(getattr(buf, name)), getattr(ref, name), err_msg=name)
        for k, (big, sent) in self.big.items():
            b = _np(big)
            assert (b[:PAD] == sent).all() and (b[PAD + self.rows:] == sent).all(), k

    def add(self, batch, done):
        self.buf.add(_dev(batch, self.gpu), torch.as_tensor(done).to(self.gpu))
        self.ref.add(batch, done)

    def sample(self, B, draws, crop_from, what='', idxs=None):
        """One injected-draw sample against the restatement."""
        d = dict(draws) if crop_from is None else dict(draws, crop_from=crop_from)
        out = self.buf.sample(B, idxs=idxs, draws=d, record_draws=True)
        exp, ix = ovn.sample(self.ref, self.cfg, draws, crop_from, hgc=self.hgc, idxs=idxs)
        _assert_batch(out, exp, what)
        names = dict(_idxs='idxs', _value_goal_idxs='vg', _actor_goal_idxs='ag')
        if self.hgc:
            names = dict(_idxs='idxs', _high_value_goal_idxs='hvg', _high_actor_goal_idxs='hag',
                         _low_value_goal_idxs='lvg')
        for key, name in names.items():
            np.testing.assert_array_equal(_np(out[key]), ix[name], err_msg=f'{what} {key}')
        for k, v in d.items():  # the record repeats what was injected
            if not (idxs is not None and k == 'pick'):
                np.testing.assert_array_equal(_np(out['_draws'][k]), v, err_msg=f'{what} draw {k}')
        assert ('crop_from' in out['_draws']) == (crop_from is not None)
        return out, ix


def _draws(rng, B, npick, hgc):
    return ohn.random_draws(rng, B, npick, True) if hgc else onp.random_draws(rng, B, npick)


FRAMES = {'u8_6x5x2': ((6, 5, 2), np.uint8), 'u8_8x8x4': ((8, 8, 4), np.uint8), 'f32_5': ((5,), np.float32),
          'f64_2': ((2,), np.float64)}


def _example(kind):
    shape, dt = FRAMES[kind]
    return dict(observations=np.zeros(shape, dt), actions=np.zeros(2, np.float32),
                next_observations=np.zeros(shape, dt))


def _rows(rng, n, kind):
    shape, dt = FRAMES[kind]

    def frames():
        if dt == np.uint8:
            return rng.randint(0, 256, (n,) + shape).astype(np.uint8)
        return rng.normal(size=(n,) + shape).astype(dt)

    return dict(observations=frames(), actions=rng.uniform(-1, 1, (n, 2)).astype(np.float32),
                next_observations=frames())


# -------------------------------------------------------------- 1. fixture replay
@pytest.mark.parametrize('cname', list(ovn.GOLDEN_CONFIGS))
def test_golden_history_samples_equal_the_reference(gpu, gold, cname):
    cfg, hgc = ovn.GOLDEN_CONFIGS[cname], ovn.HGC[cname]
    g = Guarded(ovn.EXAMPLE, ovn.N, ovn.T, cfg, gpu, hgc=hgc)
    for t in range(ovn.STEPS):
        g.add({k: gold[f'in_{k}'][t] for k in ovn.EXAMPLE}, gold['done'][t])
        S = t + 1
        if S not in ovn.SNAPS:
            continue
        pre = f's{S}_{cname}_'
        draws = {k[len(pre) + 5:]: v for k, v in gold.items() if k.startswith(pre + 'draw_')}
        out = g.buf.sample(ovn.B, draws=draws)
        keys = [k for k in gold[pre + 'keys'].tolist() if k != 'terminals']  # the snapshot's own column
        _assert_batch(out, {k: gold[pre + 'out_' + k] for k in keys}, pre)
        g.check()
        snap = g.buf.snapshot()  # unstacked frames
        assert tuple(snap['observations'].shape) == (ovn.N * min(S, ovn.T),) + ovn.FRAME


# ------------------------------------------------- 2. sweep against the restatement
SWEEP = [(kind, F, hgc) for hgc in (False, True) for kind in FRAMES for F in (1, 2, 3, 8)]


@pytest.mark.parametrize('kind,F,hgc', SWEEP, ids=[f'{k}-F{F}-{"hgc" if h else "gc"}' for k, F, h in SWEEP])
def test_sweep_against_the_restatement(gpu, kind, F, hgc):
    """Rows of 60 B (unaligned), 256 B, 20 B and 16 B; stacks of every depth
    the kernel unrolls; rings of one slot, one env, fewer slots than F and the
    designed 5 x 6; S below, at and past the wrap; batches of one, one per XCD
    lane group and 257; injected draws and crops, guarded storage."""
    rng = np.random.RandomState(sum(map(ord, kind)) + 10 * F + hgc)
    cfg = dict(HGC_CFG if hgc else GC_CFG, frame_stack=F, p_aug=1.0)
    for N, T in ((1, 1), (1, 3), (3, 2), (5, 6)):
        g = Guarded(_example(kind), N, T, cfg, gpu, hgc=hgc)
        at = {S for S in (1, T - 1, T, T + 1, 3 * T + 2) if S >= 1}
        for S in range(1, 3 * T + 3):
            g.add(_rows(rng, N, kind), rng.rand(N) < 0.3)
            if S not in at:
                continue
            for B in (1, 64, 257):
                out, _ = g.sample(B, _draws(rng, B, g.ref.L * N, hgc), ovn.crop_draws(rng, B), f'{N}x{T} S={S} B={B}')
                shape = FRAMES[kind][0]
                assert tuple(out['observations'].shape) == (B,) + shape[:-1] + (shape[-1] * F,)
                assert out['next_observations'].shape == out['observations'].shape
            g.check()  # a sample writes nothing into the ring


# ------------------------------------------------------------ 3. the LDS band path
def test_frames_over_the_lds_budget_are_staged_in_bands(gpu):
    """uint8 64 x 64 x 6 at F = 3: 73,728 B of source frames, over the 64 KB of
    dynamic LDS, so every image is composed from bands of rows; shifted by the
    crop, whose first and last source rows repeat at the band edges."""
    rng = np.random.RandomState(3)
    shape, N, T, B = (64, 64, 6), 2, 4, 8
    assert 3 * np.prod(shape) == 73728 > 64 * 1024
    ex = dict(observations=np.zeros(shape, np.uint8), next_observations=np.zeros(shape, np.uint8))
    cfg = dict(GC_CFG, frame_stack=3, p_aug=1.0)
    g = Guarded(ex, N, T, cfg, gpu)
    for S in range(1, 7):
        g.add(dict(observations=rng.randint(0, 256, (N,) + shape).astype(np.uint8),
                   next_observations=rng.randint(0, 256, (N,) + shape).astype(np.uint8)), rng.rand(N) < 0.3)
    crop_from = ovn.crop_draws(rng, B)
    crop_from[:4] = [[0, 0], [6, 6], [0, 6], [3, 3]]
    out, _ = g.sample(B, onp.random_draws(rng, B, T * N), crop_from, 'bands')
    assert tuple(out['observations'].shape) == (B, 64, 64, 18)
    g.check()


# --------------------------------------- 4. a never-done env past the ring's wrap
def test_never_done_env_is_clamped_at_its_oldest_live_row(gpu):
    """S > T with no done at all: every dead step's slot holds a newer row of
    the same env with an equal ep_seq, so only the liveness bound stops the
    stack.  The oldest live row of every env is a stack of that one frame."""
    rng = np.random.RandomState(4)
    N, T, F, S = 2, 4, 3, 7
    cfg = dict(GC_CFG, frame_stack=F, p_aug=None)
    g = Guarded(_example('u8_6x5x2'), N, T, cfg, gpu)
    hist = []
    for _ in range(S):
        rows = _rows(rng, N, 'u8_6x5x2')
        hist.append(rows['observations'])
        g.add(rows, np.zeros(N, bool))
    assert int(g.buf.cur_seq.sum()) == 0 and int(g.buf.ep_seq.sum()) == 0
    idxs = np.array([0, T, 1, T + 1, T - 1, 2 * T - 1])  # both envs: oldest, second oldest, newest
    B = len(idxs)
    out, _ = g.sample(B, onp.random_draws(rng, B, T * N), None, 'never done', idxs=idxs)
    obs = _np(out['observations'])
    for b, (e, k) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1), (0, T - 1), (1, T - 1)]):
        want = [hist[max(S - T + k - i, S - T)][e] for i in reversed(range(F))]
        np.testing.assert_array_equal(obs[b], np.concatenate(want, axis=-1), err_msg=f'env {e} offset {k}')
    # the slot before the oldest live row holds the newest step, not an older frame of the stack
    assert not np.array_equal(hist[S - 1][0], hist[S - T][0])


# ------------------------------------------------- 5. cross-checks at one (seed, call)
def _filled(cls, cfg, gpu, seed, steps=9, N=5, T=6):
    rng = np.random.RandomState(steps)
    buf = cls.create(_example('u8_6x5x2'), N, T, cfg, device=gpu, seed=seed)
    for _ in range(steps):
        buf.add(_dev(_rows(rng, N, 'u8_6x5x2'), gpu), torch.as_tensor(rng.rand(N) < 0.3).to(gpu))
    return buf


def test_crop_only_equals_gcdataset_over_the_snapshot(gpu):
    """p_aug without frame_stack: the offline sampler crops a regular dataset,
    so at one (seed, call) the whole batch is equal, the device-drawn
    crop_from included."""
    cfg = dict(GC_CFG, frame_stack=None, p_aug=1.0)
    buf = _filled(GCReplayBuffer, cfg, gpu, seed=77)
    gc = GCDataset(Dataset(buf.snapshot()), cfg, seed=77)
    for call, B in enumerate((1, 64, 257)):
        assert buf._calls == gc._calls == call
        got, exp = buf.sample(B, record_draws=True), gc.sample(B, record_draws=True)
        for k in list(buf) + ['value_goals', 'actor_goals', 'masks', 'rewards', '_idxs', '_value_goal_idxs',
                              '_actor_goal_idxs']:
            assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), (k, B)
        assert sorted(got['_draws']) == sorted(exp['_draws']) and 'crop_from' in got['_draws']
        for k in exp['_draws']:
            assert torch.equal(got['_draws'][k], exp['_draws'][k]), (k, B)
    plain = _filled(GCReplayBuffer, dict(cfg, p_aug=None), gpu, seed=77)
    plain._calls = buf._calls - 1
    raw = plain.sample(257)
    assert not torch.equal(raw['observations'], got['observations'])  # the crop moved pixels
    assert torch.equal(raw['actions'], got['actions'])


@pytest.mark.parametrize('hgc', [False, True], ids=['gc', 'hgc'])
def test_stacks_equal_the_offline_sampler_and_nothing_else_moves(gpu, hgc):
    """With frame_stack: the offline sampler over the snapshot minus
    next_observations, fed the ring's recorded idxs and draws, stacks and crops
    the same observations and goals; and the indices, draws and non-image keys
    are those of the same buffer without the two keys at the same seed and
    call, which issues the one launch it always did."""
    cls = HGCReplayBuffer if hgc else GCReplayBuffer
    cfg = dict(HGC_CFG if hgc else GC_CFG, frame_stack=3, p_aug=1.0)
    buf = _filled(cls, cfg, gpu, seed=5)
    plain = _filled(cls, dict(cfg, frame_stack=None, p_aug=None), gpu, seed=5)
    assert 'sample' in vars(buf) and 'sample' not in vars(plain)
    B = 257
    got, base = buf.sample(B, record_draws=True), plain.sample(B, record_draws=True)
    image = [k for k in got if not k.startswith('_') and got[k].dim() == 4]
    assert len(image) == (16 if hgc else 4)  # HGCDataset._VISUAL_KEYS and the two aliases among them
    for k in base:
        if k == '_draws':
            for d in base[k]:
                assert torch.equal(got[k][d], base[k][d]), d
        elif k not in image and k != 'high_value_reps':
            assert torch.equal(got[k], base[k]), k
    if not hgc:
        snap = {k: v for k, v in buf.snapshot().items() if k != 'next_observations'}
        gc = GCDataset(Dataset(snap), cfg, seed=5)
        draws = {k: v for k, v in got['_draws'].items() if k != 'pick'}
        exp = gc.sample(B, idxs=got['_idxs'], draws=draws)
        for k in ('observations', 'value_goals', 'actor_goals'):
            assert exp[k].shape == (B, 6, 5, 6) and torch.equal(got[k], exp[k]), k


# ------------------------------------------------------------------- 6. the coin
def test_coin_and_crop_offsets(gpu):
    cfg = dict(GC_CFG, frame_stack=2, p_aug=0.5)
    buf = _filled(GCReplayBuffer, cfg, gpu, seed=11)
    still = _filled(GCReplayBuffer, dict(cfg, p_aug=0.0), gpu, seed=11)
    none = _filled(GCReplayBuffer, dict(cfg, p_aug=None), gpu, seed=11)
    np.random.seed(123)
    state = np.random.get_state()

    def untouched():
        now = np.random.get_state()
        return now[2] == state[2] and np.array_equal(now[1], state[1])

    a = buf.sample(64, evaluation=True, record_draws=True)
    b = still.sample(64, record_draws=True)
    c = none.sample(64, record_draws=True)
    assert untouched()  # no coin under evaluation, nor with p_aug 0 or None
    for o in (a, b, c):
        assert 'crop_from' not in o['_draws']
    for k in a:
        if k != '_draws':
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    # one coin per call otherwise, whichever way it falls
    after = np.random.RandomState(123)
    coins = after.rand(6) < 0.5
    assert coins.any() and not coins.all()
    held = None
    for i, coin in enumerate(coins):
        if i % 2:
            assert ('crop_from' in buf.sample(64, record_draws=True)['_draws']) == bool(coin), i
        else:
            held = buf.sample(64, out=held)
    now, want = np.random.get_state(), after.get_state()
    assert now[2] == want[2] and np.array_equal(now[1], want[1])
    # the device draw reaches all 49 offset pairs, each in [0, 6]^2
    crop = _filled(GCReplayBuffer, dict(cfg, p_aug=1.0), gpu, seed=11)
    cf = _np(crop.sample(4096, record_draws=True)['_draws']['crop_from'])
    assert cf.shape == (4096, 2) and cf.min() == 0 and cf.max() == 6
    assert len({tuple(r) for r in cf.tolist()}) == 49


@pytest.mark.parametrize('hgc', [False, True], ids=['gc', 'hgc'])
def test_state_observations_with_p_aug_draw_the_coin_and_nothing_else(gpu, hgc):
    """GCDataset's rule: p_aug > 0 draws the coin whether or not a key can be
    cropped; 2-D observations without frame_stack have no image column, so the
    batch is the plain buffer's and no second launch is issued."""
    cls = HGCReplayBuffer if hgc else GCReplayBuffer
    cfg = dict(HGC_CFG if hgc else GC_CFG, frame_stack=None, p_aug=0.5)
    rng = np.random.RandomState(6)
    bufs = [cls.create(_example('f32_5'), 3, 4, c, device=gpu, seed=2) for c in (cfg, dict(cfg, p_aug=None))]
    for _ in range(6):
        rows, done = _dev(_rows(rng, 3, 'f32_5'), gpu), torch.as_tensor(rng.rand(3) < 0.3).to(gpu)
        for b in bufs:
            b.add(rows, done)
    live, plain = bufs
    assert live._p_aug_live and not live._visual and 'sample' not in vars(plain)
    np.random.seed(9)
    for B in (1, 64):
        got, exp = live.sample(B, record_draws=True), plain.sample(B, record_draws=True)
        assert list(got) == list(exp) and 'crop_from' not in got['_draws']
        for k in exp:
            if k != '_draws':
                assert got[k].shape == exp[k].shape and torch.equal(got[k], exp[k]), k
    live.sample(64, evaluation=True)
    spent = np.random.RandomState(9)
    spent.rand(2)  # one coin per non-evaluation call
    assert np.random.get_state()[2] == spent.get_state()[2] and np.array_equal(np.random.get_state()[1],
                                                                               spent.get_state()[1])


# ------------------------------------------------------------ 7. the out= refill
@pytest.mark.parametrize('hgc', [False, True], ids=['gc', 'hgc'])
def test_out_refills_in_place(gpu, hgc):
    cls = HGCReplayBuffer if hgc else GCReplayBuffer
    cfg = dict(HGC_CFG if hgc else GC_CFG, frame_stack=3, p_aug=0.5)
    a, b = (_filled(cls, cfg, gpu, seed=9) for _ in range(2))
    coins = np.random.RandomState(31).rand(4) < 0.5
    assert coins.any() and not coins.all()  # the refills crop and do not crop
    np.random.seed(31)
    fresh = [{k: v.clone() for k, v in a.sample(64).items()} for _ in range(4)]
    assert not torch.equal(fresh[0]['observations'], fresh[1]['observations'])
    np.random.seed(31)
    out = b.sample(64)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    assert all(torch.equal(out[k], fresh[0][k]) for k in fresh[0])
    for want in fresh[1:]:
        again = b.sample(64, out=out)
        assert again is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
        for k in want:
            assert torch.equal(out[k], want[k]), k
    spent = np.random.RandomState(31)
    spent.rand(4)  # a coin per call, refills included
    assert np.random.get_state()[2] == spent.get_state()[2] and np.array_equal(np.random.get_state()[1],
                                                                               spent.get_state()[1])
    with pytest.raises(ValueError, match='64 samples'):  # another batch size
        b.sample(32, out=out)


# ---------------------------------------------------------------- 8. end to end
def test_powderworld_steps_through_add_step(gpu):
    """powderworld-easy, 4 envs, a ring of 8 slots, 12 steps: the step's
    observation is the episode's last where it ended (final_observation) and
    the masked reset's is the next row's; F = 3 stacks and crops equal the
    restatement fed the same step outputs."""
    n, T, steps, F, B = 4, 8, 12, 3, 64
    env = ogbench_amd.make('powderworld-easy-v0', num_envs=n, device=gpu, max_episode_steps=5)
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
        final, _, term, trunc, _ = env.step(act)
        final, term, trunc = final.clone(), term.clone(), trunc.clone()
        done = term | trunc
        obs = env.reset(mask=done)[0] if bool(done.any()) else final
        buf.add_step(prev, act, term, trunc, obs, final)
        ref.add_step(_np(prev), _np(act), _np(term), _np(trunc), _np(obs), _np(final))
        ends += int(done.sum())
    assert ends >= 2 * n and buf.steps == steps > T
    for k, v in ref.cols.items():
        np.testing.assert_array_equal(_np(buf[k]), v, err_msg=k)
    rng = np.random.RandomState(8)
    draws, crop_from = onp.random_draws(rng, B, T * n), ovn.crop_draws(rng, B)
    out = buf.sample(B, draws=dict(draws, crop_from=crop_from))
    exp, _ = ovn.sample(ref, cfg, draws, crop_from)
    _assert_batch(out, exp, 'powderworld')
    assert tuple(out['observations'].shape) == (B, 32, 32, 18)
    env.close()
