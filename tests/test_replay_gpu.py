"""GPU tests of the replay buffer (replay_insert_kernel / replay_sample_kernel
via include/ogbx_replay.h, ogbench_amd.datasets.ReplayBuffer): bit for bit
against the reference's recorded behaviour (tests/golden/replay_golden.npz) and
the NumPy restatement (tests/replay_np.py)."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ogbench_amd
import replay_np as rnp
from ogbench_amd import _lib
from ogbench_amd import datasets as D
from ogbench_amd.datasets import Dataset, ReplayBuffer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'replay_golden.npz')
PAD = 8  # margin rows on both sides of every destination column
SENT_F, SENT_I = -7.0, 0x5A


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _np(t):
    return t.cpu().numpy()


def _readback(rb):
    """(pointer, size) as the device header holds them."""
    h = _np(rb._hdr)
    return int(h[2 * rb._parity]), int(h[2 * rb._parity + 1])


def _assert_state(rb, ref, mirrored=True):
    if mirrored:  # the host mirror, without a read-back
        assert rb._known and (rb._h_pointer, rb._h_size) == (ref.pointer, ref.size)
    assert _readback(rb) == (ref.pointer, ref.size)
    assert (rb.pointer, rb.size) == (ref.pointer, ref.size)


def _assert_cols(rb, ref):
    for k, v in ref.cols.items():
        got = _np(rb[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (k, got.dtype, got.shape)
        np.testing.assert_array_equal(got, v, err_msg=k)


def _assert_batch(out, exp):
    assert [k for k in out if not k.startswith('_')] == list(exp)
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (k, got.dtype, got.shape, v.dtype, v.shape)
        np.testing.assert_array_equal(got, v, err_msg=k)


class Guarded:
    """A ReplayBuffer whose columns are the middle rows of sentinel-filled
    tensors, and its restatement; the margins must keep their sentinels."""

    def __init__(self, example, max_size, gpu, seed=1):
        self.big, cols = {}, {}
        for k, v in example.items():
            v = np.array(v)
            sent = SENT_F if v.dtype.kind == 'f' else SENT_I
            big = torch.full((max_size + 2 * PAD,) + v.shape, sent, dtype=torch.from_numpy(np.zeros(0, v.dtype)).dtype,
                             device=gpu)
            big[PAD:PAD + max_size] = 0
            self.big[k] = (big, sent)
            cols[k] = big[PAD:PAD + max_size]
        self.rb = ReplayBuffer(cols, device=gpu, seed=seed)
        for k in cols:  # the buffer writes into the guarded storage itself
            assert self.rb[k].data_ptr() == cols[k].data_ptr()
        self.ref = rnp.ReplayNp.create(example, max_size)
        self.max_size = max_size

    def check(self, mirrored=True):
        _assert_state(self.rb, self.ref, mirrored)
        _assert_cols(self.rb, self.ref)
        for k, (big, sent) in self.big.items():
            b = _np(big)
            assert (b[:PAD] == sent).all() and (b[PAD + self.max_size:] == sent).all(), k

    def add(self, batch, keep=None, mirrored=None):
        dev = self.rb.device
        self.rb.add_transitions({k: torch.as_tensor(v).to(dev) for k, v in batch.items()},
                                None if keep is None else torch.as_tensor(keep).to(dev))
        self.ref.add_transitions(batch, keep)
        self.check(keep is None if mirrored is None else mirrored)


SAC = dict(observations=np.zeros(3, np.float32), actions=np.zeros(2, np.float32), rewards=0.0, masks=1.0,
           next_observations=np.zeros(3, np.float32))


def _sac_rows(rng, n):
    return dict(observations=rng.normal(size=(n, 3)).astype(np.float32),
                actions=rng.uniform(-1, 1, (n, 2)).astype(np.float32), rewards=rng.normal(size=n),
                masks=(rng.rand(n) < 0.8).astype(np.float64),
                next_observations=rng.normal(size=(n, 3)).astype(np.float32))


# -------------------------------------------------------------------- inserts
def test_add_transition_against_the_golden_ring(gpu, gold):
    rows = rnp.scenario(gold, 'ring5', 'in')
    snaps = rnp.scenario(gold, 'ring5', 'snap')
    rb = ReplayBuffer.create({k: v[0] for k, v in rows.items()}, 5, device=gpu)
    assert rb.max_size == 5 and (rb.pointer, rb.size) == (0, 0)
    assert [rb[k].dtype for k in rows] == [torch.from_numpy(v).dtype for v in snaps.values()]
    for i in range(7):
        rb.add_transition({k: v[i] for k, v in rows.items()})
        want = (int(gold['ring5_pointer'][i + 1]), int(gold['ring5_size'][i + 1]))
        assert (rb._h_pointer, rb._h_size) == want and _readback(rb) == want
        for k in rows:
            np.testing.assert_array_equal(_np(rb[k]), snaps[k][i], err_msg=f'{k} after add {i}')
    assert (rb.pointer, rb.size) == (2, 4)  # the reference's size quirk
    rb.clear()
    assert (rb.pointer, rb.size) == tuple(gold['clear_state']) == _readback(rb)
    assert str(gold['clear_error']) == 'ValueError'
    with pytest.raises(ValueError):
        rb.sample(4)
    for k in rows:  # clear() leaves the rows
        np.testing.assert_array_equal(_np(rb[k]), snaps[k][6])


def test_python_scalars_create_float64_columns(gpu):
    rb = ReplayBuffer.create(dict(observations=np.zeros(2, np.float32), rewards=0.0, masks=1.0, steps=3), 4,
                             device=gpu)
    assert [rb[k].dtype for k in rb] == [torch.float32, torch.float64, torch.float64, torch.int64]
    assert [tuple(rb[k].shape) for k in rb] == [(4, 2), (4,), (4,), (4,)]
    assert all(int(rb[k].abs().sum()) == 0 for k in rb)


def test_add_transition_casts_as_numpy_assignment(gpu, gold):
    buf = rnp.scenario(gold, 'dtypes', 'buf')
    rb = ReplayBuffer.create(dict(a64=np.zeros(2), b32=np.zeros(3, np.float32), pyfloat=0.0,
                                  image=np.zeros((4, 4, 3), np.uint8), count=np.int64(0)), 5, device=gpu)
    for i in range(4):
        rb.add_transition(rnp.scenario(gold, 'dtypes', f'add{i}'))
    assert (rb.pointer, rb.size) == (4, 4)
    for k, v in buf.items():
        got = _np(rb[k])
        assert got.dtype == v.dtype
        np.testing.assert_array_equal(got, v, err_msg=k)


@pytest.mark.parametrize('n', [63, 65, 257])
def test_batched_inserts_cross_wave_and_tile_edges(gpu, n):
    g = Guarded(SAC, 300, gpu)
    rng = np.random.RandomState(n)
    for _ in range(700 // n + 1):  # through the wrap, up to the size plateau
        g.add(_sac_rows(rng, n))
    assert g.ref.size == 299


def test_wrap_inside_a_tile(gpu):
    g = Guarded(SAC, 300, gpu)
    g.rb.pointer = g.ref.pointer = 290
    g.rb.size = g.ref.size = 290
    g.check()
    g.add(_sac_rows(np.random.RandomState(0), 100))  # rows 0..9 fill 290..299, rows 10.. wrap to 0
    assert (g.ref.pointer, g.ref.size) == (90, 299)


def test_n_equal_to_max_size_and_one_more(gpu):
    g = Guarded(SAC, 300, gpu)
    rng = np.random.RandomState(1)
    g.add(_sac_rows(rng, 7))
    g.add(_sac_rows(rng, 300))
    assert (g.ref.pointer, g.ref.size) == (7, 299)
    with pytest.raises(ValueError, match='max_size'):
        g.rb.add_transitions({k: torch.as_tensor(v).to(gpu) for k, v in _sac_rows(rng, 301).items()})
    g.check()  # refused on the host: nothing moved
    with pytest.raises(ValueError, match='keys'):
        g.rb.add_transitions(dict(observations=torch.zeros(1, 3, device=gpu)))
    with pytest.raises(ValueError, match='valids'):
        ReplayBuffer(dict(observations=torch.zeros(4, 2), valids=torch.ones(4)), device=gpu)


ROWS = dict(b1=np.uint8(0), b4=np.float32(0), b8=np.float64(0), b12=np.zeros(3, np.float32), b16=np.zeros(2),
            ant=np.zeros(29), image=np.zeros((4, 4, 3), np.uint8))


def _row_batch(rng, n):
    out = {}
    for k, v in ROWS.items():
        v = np.array(v)
        out[k] = (rng.randint(0, 256, (n,) + v.shape).astype(np.uint8) if v.dtype == np.uint8
                  else rng.normal(size=(n,) + v.shape).astype(v.dtype))
    return out


def test_row_sizes_1_to_232_bytes(gpu):
    """Rows of 1, 4, 8, 12, 16, 232 and 48 bytes; the guarded columns start at
    PAD rows into their storage, so the 12-byte column is only 4-byte aligned."""
    g = Guarded(ROWS, 300, gpu)
    assert [g.rb[k][0].numel() * g.rb[k].element_size() for k in ROWS] == [1, 4, 8, 12, 16, 232, 48]
    rng = np.random.RandomState(2)
    g.add(_row_batch(rng, 257))
    g.add(_row_batch(rng, 65))  # wraps
    keep = rng.rand(257) < 0.5
    g.add(_row_batch(rng, 257), keep)


def test_wide_rows_take_the_16_row_tiles(gpu):
    """The launch halves its rows per workgroup from 256 while a workgroup
    still moves 16 KB or more: 32 for the 321-byte rows above, 16 (the floor)
    for these 1,608-byte ones, with and without a mask and through the wrap."""
    ex = dict(wide=np.zeros(200), tag=np.int64(0))
    g = Guarded(ex, 300, gpu)
    rng = np.random.RandomState(8)
    rows = lambda n: dict(wide=rng.normal(size=(n, 200)), tag=rng.randint(0, 1 << 40, n))  # noqa: E731
    g.add(rows(257))
    g.add(rows(65), rng.rand(65) < 0.5)
    g.add(rows(257), rng.rand(257) < 0.7)
    g.add(rows(17))


DST = dict(u8=np.uint8, i32=np.int32, i64=np.int64, f32=np.float32, f64=np.float64)


def _values(rng, src, dst, shape):
    """In-range values of dtype ``src`` for a column of dtype ``dst``."""
    if src == np.bool_:
        return rng.rand(*shape) < 0.5
    lo = 0 if (src == np.uint8 or dst == np.uint8) else -100
    if np.dtype(src).kind == 'f':
        return rng.uniform(lo, 100, shape).astype(src)  # fractions: truncation and float64 -> float32 rounding
    return rng.randint(lo, 101, shape).astype(src)


@pytest.mark.parametrize('src', [np.bool_, np.uint8, np.int32, np.int64, np.float32, np.float64],
                         ids=lambda d: np.dtype(d).name)
def test_every_source_dtype_into_every_column_dtype(gpu, src):
    example = {k: np.zeros(3, d) for k, d in DST.items()}
    g = Guarded(example, 300, gpu)
    rng = np.random.RandomState(3)
    n = 257
    g.add({k: _values(rng, src, d, (n, 3)) for k, d in DST.items()})
    # one_minus: 1 - value in the column's dtype, after the cast
    batch = {k: _values(rng, src, d, (40, 3)) for k, d in DST.items()}
    dev = {k: torch.as_tensor(v).to(gpu) for k, v in batch.items()}
    g.rb._insert([(k, dev[k], None, D.REPLAY_OP_ONE_MINUS) for k in g.rb], 40, None, None)
    with np.errstate(all='ignore'):
        g.ref.add_transitions({k: (1 - v.astype(DST[k])).astype(DST[k]) for k, v in batch.items()})
    g.check()


def test_keep_all_zero_is_a_noop_and_all_one_is_no_mask(gpu):
    g = Guarded(SAC, 300, gpu)
    rng = np.random.RandomState(4)
    g.add(_sac_rows(rng, 65))
    before = _readback(g.rb)
    g.add(_sac_rows(rng, 257), np.zeros(257, bool))
    assert _readback(g.rb) == before == (65, 65)
    g.add(_sac_rows(rng, 257), np.ones(257, np.uint8))
    assert (g.ref.pointer, g.ref.size) == (22, 299)


@pytest.mark.parametrize('n,max_size,start', [(257, 300, 0), (1000, 1024, 900)])
def test_keep_with_holes_across_tile_edges(gpu, n, max_size, start):
    g = Guarded(SAC, max_size, gpu)
    g.rb.pointer = g.ref.pointer = start
    g.rb.size = g.ref.size = start
    rng = np.random.RandomState(n)
    keep = rng.rand(n) < 0.6
    for edge in range(256, n, 256):  # holes and runs that straddle the workgroup tiles
        keep[edge - 9:edge + 5] = False
        keep[edge + 5:edge + 8] = True
    keep[-1] = True
    # a mask that starts 3 bytes into its storage: the count's unaligned head and tail
    store = torch.zeros(n + 7, dtype=torch.bool, device=gpu)
    store[3:3 + n] = torch.as_tensor(keep)
    rows = _sac_rows(rng, n)
    g.rb.add_transitions({k: torch.as_tensor(v).to(gpu) for k, v in rows.items()}, store[3:3 + n])
    assert not g.rb._known  # the host does not know how many rows were kept
    g.ref.add_transitions(rows, keep)
    g.check(mirrored=False)
    assert g.rb._known  # the properties read the header back
    g.add(_sac_rows(rng, 65), rng.rand(65) < 0.5)
    g.add(_sac_rows(rng, 63))


# ------------------------------------------------------------------- add_step
def test_add_step_against_the_restatement(gpu):
    n = 257
    ex = dict(observations=np.zeros(4), actions=np.zeros(2, np.float32), rewards=0.0, masks=1.0,
              next_observations=np.zeros(4))
    g = Guarded(ex, 300, gpu)
    rng = np.random.RandomState(6)
    for rnd in range(3):
        obs, nxt, fin = rng.normal(size=(3, n, 4))
        act = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        rew = rng.normal(size=n).astype(np.float32)  # float32 rewards into the float64 column
        term = rng.rand(n) < 0.2
        done = np.arange(n) % 3 == rnd  # a third of the rows
        keep = None if rnd < 2 else rng.rand(n) < 0.7
        t = lambda a: torch.as_tensor(a).to(gpu)  # noqa: E731
        g.rb.add_step(t(obs), t(act), t(rew), t(term), t(nxt), t(fin), t(done), None if keep is None else t(keep))
        g.ref.add_step(obs, act, rew, term, nxt, fin, done, keep)
        g.check(mirrored=keep is None)
    with pytest.raises(ValueError, match='go together'):
        g.rb.add_step(t(obs), t(act), t(rew), t(term), t(nxt), t(fin))


def test_add_step_on_a_real_auto_reset_env(gpu):
    n, steps = 64, 13
    env = ogbench_amd.make('pointmaze-medium-v0', num_envs=n, device=gpu, auto_reset=True, max_episode_steps=5)
    obs, _ = env.reset(seed=3)
    ex = dict(observations=np.zeros(obs.shape[1:]), actions=np.zeros(2, np.float32), rewards=0.0, masks=1.0,
              next_observations=np.zeros(obs.shape[1:]))
    rb = ReplayBuffer.create(ex, 700, device=gpu)
    host = {k: torch.zeros_like(v) for k, v in rb.items()}  # the torch-op composition
    gen = torch.Generator().manual_seed(9)
    ended = 0
    for t in range(steps):
        prev = obs.clone()  # the env's observation view is overwritten by the step
        act = (torch.rand(n, 2, generator=gen) * 2 - 1).float().to(gpu)
        obs, rew, term, trunc, info = env.step(act)
        done = term | trunc
        rb.add_step(prev, act, rew, term, obs, info['final_observation'], done)
        at = (torch.arange(n, device=gpu) + t * n) % 700
        host['observations'].index_copy_(0, at, prev)
        host['actions'].index_copy_(0, at, act)
        host['rewards'].index_copy_(0, at, rew.to(torch.float64))
        host['masks'].index_copy_(0, at, 1.0 - term.to(torch.float64))
        host['next_observations'].index_copy_(0, at, torch.where(done[:, None], info['final_observation'], obs))
        ended += int(done.sum())
        if done.any():  # the reset observation is not the episode's last
            assert not torch.equal(obs[done], info['final_observation'][done])
    assert ended >= n  # every env ended an episode at least once
    assert (rb.pointer, rb.size) == ((steps * n) % 700, 699)
    for k in host:
        assert torch.equal(rb[k], host[k]), k


# ------------------------------------------------------------------- sampling
def _golden_buffer(gold, name, gpu, seed=1):
    cols = rnp.scenario(gold, name, 'buf')
    pointer, size = gold[f'{name}_state'].tolist()
    rb = ReplayBuffer(cols, device=gpu, seed=seed)
    rb.pointer, rb.size = pointer, size
    return rb


@pytest.mark.parametrize('name', ['sample_regular', 'sample_compact'])
def test_sample_with_the_recorded_draws(gpu, gold, name):
    rb = _golden_buffer(gold, name, gpu)
    assert rb.size == 120 < rb.max_size
    out = rb.sample(64, idxs=gold[f'{name}_idxs'])
    assert list(out) == gold[f'{name}_keys'].tolist()
    _assert_batch(out, rnp.scenario(gold, name, 'out'))
    # rows up to size - 1 while size < max_size: the compact clamp is the current size - 1
    sub = gold[f'{name}_sub_idxs']
    assert sub.max() == rb.size - 1
    _assert_batch(rb.get_subset(torch.as_tensor(sub).to(gpu)), rnp.scenario(gold, name, 'sub_out'))


def test_full_initial_dataset_samples_every_row_and_refuses_adds(gpu, gold):
    for n in (3, 4, 5):
        init = rnp.scenario(gold, f'init{n}', 'in')
        rb = ReplayBuffer.create_from_initial_dataset(init, 5, device=gpu)
        assert (rb.pointer, rb.size) == (n, n) == _readback(rb)
        one = {k: torch.as_tensor(v).to(gpu) for k, v in rnp.scenario(gold, f'init{n}', 'add').items()}
        if n == 5:
            _assert_batch(rb.sample(16, idxs=gold['init5_idxs']), rnp.scenario(gold, 'init5', 'out'))
            assert str(gold['init5_error']) == 'IndexError'
            with pytest.raises(IndexError):
                rb.add_transitions(one)
        else:
            rb.add_transitions(one)
            assert (rb.pointer, rb.size) == (int(gold[f'init{n}_pointer'][1]), int(gold[f'init{n}_size'][1]))
        for k, v in rnp.scenario(gold, f'init{n}', 'buf').items():
            np.testing.assert_array_equal(_np(rb[k]), v, err_msg=k)


@pytest.mark.parametrize('compact', [False, True], ids=['regular', 'compact'])
@pytest.mark.parametrize('size', [1, 2, 299])
def test_philox_draws_equal_dataset_sample_over_the_snapshot(gpu, size, compact):
    rng = np.random.RandomState(size)
    # Dataset.sample drops columns named 'masks' / 'rewards' (its sampler's own
    # scalar keys), so the SAC columns go under other names here
    names = dict(observations='observations', actions='actions', rewards='returns', masks='flags',
                 next_observations='next_observations')
    if compact:
        del names['next_observations']
    rb = ReplayBuffer.create({new: SAC[old] for old, new in names.items()}, 300, device=gpu, seed=77)
    sac = _sac_rows(rng, size)
    rb.add_transitions({new: torch.as_tensor(sac[old]).to(gpu) for old, new in names.items()})
    assert rb.size == size
    snap = Dataset({k: v[:size].clone() for k, v in rb.items()}, device=gpu)
    snap._sampler()._seed = 77
    for call, batch in enumerate((1, 64, 257)):
        assert rb._calls == snap._sampler()._calls == call
        got = rb.sample(batch, record_idxs=True)
        exp = snap.sample(batch)
        idxs = _np(got.pop('_idxs'))
        assert idxs.min() >= 0 and idxs.max() < size
        assert list(got) == list(exp)
        for k in exp:
            assert got[k].dtype == exp[k].dtype and torch.equal(got[k], exp[k]), (k, batch)
    if size == 299:
        assert len(np.unique(idxs)) > 100


def test_out_refills_in_place(gpu, gold):
    a = _golden_buffer(gold, 'sample_compact', gpu, seed=5)
    b = _golden_buffer(gold, 'sample_compact', gpu, seed=5)
    first = {k: v.clone() for k, v in a.sample(64).items()}
    second = {k: v.clone() for k, v in a.sample(64).items()}
    assert not torch.equal(first['observations'], second['observations'])
    out = b.sample(64)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    assert all(torch.equal(out[k], first[k]) for k in first)
    again = b.sample(64, out=out)
    assert again is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
    assert all(torch.equal(out[k], second[k]) for k in second)
    assert b.sample(32, out=out) is not out  # another batch size: a new batch


def test_empty_draws_after_a_masked_insert_into_an_empty_buffer(gpu):
    rb = ReplayBuffer.create(SAC, 300, device=gpu, seed=2)
    rows = {k: torch.as_tensor(v).to(gpu) for k, v in _sac_rows(np.random.RandomState(0), 65).items()}
    assert rb.empty_draws() == 0
    rb.add_transitions(rows, torch.zeros(65, dtype=torch.bool, device=gpu))
    assert not rb._known
    out = rb.sample(8, record_idxs=True)  # the host cannot know: row 0, counted
    assert rb.empty_draws() == 8
    assert _np(out['_idxs']).tolist() == [0] * 8
    assert all(int(v.abs().sum()) == 0 for v in out.values())
    assert rb.size == 0 and rb._known
    with pytest.raises(ValueError):
        rb.sample(8)
    assert rb.empty_draws() == 8


def test_twenty_rounds_of_insert_and_sample_without_a_sync(gpu):
    max_size, n, rounds = 300, 37, 20
    ex = {k: v for k, v in SAC.items() if k != 'next_observations'}  # compact: next is clamped at the size of its round
    rb = ReplayBuffer.create(ex, max_size, device=gpu, seed=11)
    rng = np.random.RandomState(12)
    host_rows = [{k: v for k, v in _sac_rows(rng, n).items() if k in ex} for _ in range(rounds)]
    host_keep = [None if r % 3 == 0 else rng.rand(n) < 0.7 for r in range(rounds)]
    dev_rows = [{k: torch.as_tensor(v).to(gpu) for k, v in rows.items()} for rows in host_rows]
    dev_keep = [None if k is None else torch.as_tensor(k).to(gpu) for k in host_keep]
    torch.cuda.synchronize()
    outs = []
    for r in range(rounds):  # nothing below reads anything back
        rb.add_transitions(dev_rows[r], dev_keep[r])
        outs.append(rb.sample(64, record_idxs=True))
    assert not rb._known
    ref = rnp.ReplayNp.create(ex, max_size)
    for r in range(rounds):
        ref.add_transitions(host_rows[r], host_keep[r])
        idxs = _np(outs[r].pop('_idxs'))
        assert idxs.min() >= 0 and idxs.max() < ref.size, r
        _assert_batch(outs[r], ref.get_subset(idxs))
    assert (rb.pointer, rb.size) == (ref.pointer, ref.size)
    assert ref.size == max_size - 1 and rb.empty_draws() == 0
    _assert_cols(rb, ref)


# ------------------------------------------------------------------------ ABI
def test_api_version_equals_the_header_constant(gpu):
    L = D._bind()
    text = open(os.path.join(ROOT, 'include', 'ogbx_replay.h')).read()
    want = int(re.search(r'#define\s+OGBX_REPLAY_API_VERSION\s+(\d+)', text).group(1))
    assert L.ogbx_replay_api_version() == want
    assert D.REPLAY_MAX_COLS == int(re.search(r'#define\s+OGBX_REPLAY_MAX_COLS\s+(\d+)', text).group(1))


def test_einval_before_any_device_work(gpu):
    L = D._bind()
    n, max_size = 8, 16
    hdr = torch.tensor([3, 3, 3, 3], dtype=torch.int64, device=gpu)
    dst = torch.full((max_size, 2), SENT_F, dtype=torch.float32, device=gpu)
    src = torch.ones(n, 2, dtype=torch.float32, device=gpu)
    keep = torch.ones(n, dtype=torch.uint8, device=gpu)
    host = (ctypes.c_int64 * 64)()
    host_ptr = ctypes.addressof(host)
    stream = _lib.stream_of(gpu)

    def col(dst_p=dst.data_ptr(), src_p=src.data_ptr(), alt=None, elems=2, sdt=4, ddt=4, op=0):
        return D.ReplayInsertColumn(dst_p, src_p, alt, elems, sdt, ddt, op, 0)

    def insert(header=hdr.data_ptr(), parity=0, ms=max_size, cols=(col(),), ncols=None, rows=n, kp=None, sel=None):
        arr = (D.ReplayInsertColumn * max(len(cols), 1))(*cols) if cols is not None else None
        return L.ogbx_replay_insert(header, parity, ms, arr, len(cols) if ncols is None else ncols, rows, kp, sel,
                                    stream)

    bad_inserts = dict(
        null_header=dict(header=None), null_cols=dict(cols=None, ncols=1), parity=dict(parity=2),
        n_zero=dict(rows=0), n_negative=dict(rows=-1), max_size_zero=dict(ms=0), n_over_max_size=dict(rows=max_size + 1),
        no_columns=dict(cols=(), ncols=0), too_many_columns=dict(cols=(col(),) * 17),
        null_dst=dict(cols=(col(dst_p=None),)), null_src=dict(cols=(col(src_p=None),)),
        row_elems_zero=dict(cols=(col(elems=0),)), row_over_4_mib=dict(cols=(col(elems=(1 << 19) + 1),)),
        src_dtype=dict(cols=(col(sdt=6),)),
        src_dtype_negative=dict(cols=(col(sdt=-1),)), dst_dtype_bool=dict(cols=(col(ddt=0),)),
        dst_dtype=dict(cols=(col(ddt=9),)), op=dict(cols=(col(op=2),)),
        alt_without_select=dict(cols=(col(alt=src.data_ptr()),)),
        host_header=dict(header=host_ptr), host_src=dict(cols=(col(src_p=host_ptr),)),
        host_dst=dict(cols=(col(dst_p=host_ptr),)), host_keep=dict(kp=host_ptr),
        host_alt=dict(cols=(col(alt=host_ptr),), sel=keep.data_ptr()),
    )
    for name, kw in bad_inserts.items():
        assert insert(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_replay_insert' in _lib.last_error(), name

    out = torch.full((n, 2), SENT_F, dtype=torch.float32, device=gpu)
    idx = torch.zeros(n, dtype=torch.int64, device=gpu)

    def gcol(src_p=dst.data_ptr(), dst_p=out.data_ptr(), rb=8, select=0, stride=0):
        return D.GcColumn(src_p, dst_p, rb, select, stride)

    def sample(header=hdr.data_ptr(), parity=0, ms=max_size, cols=(gcol(),), ncols=None, total=n, idxs=None,
               idxs_out=None, empty=None):
        arr = (D.GcColumn * max(len(cols), 1))(*cols) if cols is not None else None
        return L.ogbx_replay_sample(header, parity, ms, arr, len(cols) if ncols is None else ncols, total, idxs, 1, 0,
                                    idxs_out, empty, stream)

    bad_samples = dict(
        null_header=dict(header=None), null_cols=dict(cols=None, ncols=1), parity=dict(parity=-1),
        total_zero=dict(total=0), max_size_zero=dict(ms=0), no_columns=dict(cols=(), ncols=0),
        too_many_columns=dict(cols=(gcol(),) * 17), null_src=dict(cols=(gcol(src_p=None),)),
        null_dst=dict(cols=(gcol(dst_p=None),)), row_bytes=dict(cols=(gcol(rb=0),)), select=dict(cols=(gcol(select=2),)),
        stride=dict(cols=(gcol(stride=4),)), host_header=dict(header=host_ptr),
        host_src=dict(cols=(gcol(src_p=host_ptr),)), host_dst=dict(cols=(gcol(dst_p=host_ptr),)),
        host_idxs=dict(idxs=host_ptr), host_idxs_out=dict(idxs_out=host_ptr), host_empty=dict(empty=host_ptr),
    )
    for name, kw in bad_samples.items():
        assert sample(**kw) == _lib.OGBX_EINVAL, name
        assert 'ogbx_replay_sample' in _lib.last_error(), name
    assert L.ogbx_replay_clear(None, stream) == _lib.OGBX_EINVAL
    assert L.ogbx_replay_clear(host_ptr, stream) == _lib.OGBX_EINVAL

    # nothing was launched: header, column and batch are as they were
    torch.cuda.synchronize()
    assert _np(hdr).tolist() == [3, 3, 3, 3]
    assert bool((dst == SENT_F).all()) and bool((out == SENT_F).all()) and all(v == 0 for v in host)
    # and the same arguments, valid, do work
    assert insert(kp=keep.data_ptr()) == _lib.OGBX_OK
    assert sample(parity=1, idxs=idx.data_ptr()) == _lib.OGBX_OK
    torch.cuda.synchronize()
    assert _np(hdr).tolist() == [3, 3, 11, 11]
    assert bool((dst[3:11] == 1).all()) and bool((dst[:3] == SENT_F).all()) and bool((dst[11:] == SENT_F).all())
    assert torch.equal(out, dst[:1].expand(n, 2))
