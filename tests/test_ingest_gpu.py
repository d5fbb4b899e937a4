"""GPU: the dataset ingest kernels (csrc/loader.hip) and the load_dataset /
relabel_dataset / add_oracle_reps path of ogbench_amd/utils.py at their edges,
bit for bit against the reference's own outputs (tests/golden/ingest_golden.npz)
and against NumPy indexing.

Lane width of ogbx_gather_rows.  The library copies rows in the widest unit W
of {16, 8, 4, 1} bytes such that row_bytes % W == 0 and (src | dst) % W == 0.
The branch cannot be observed from outside, so the matrix below reaches each
one by construction: src and dst lie at the given byte offsets inside one
allocation whose base is 256-aligned (asserted), so the library is bound to
choose the listed width, and every access it then makes is aligned for it.

    row_bytes \\ (src_off, dst_off)   (0,0) (8,8) (4,4) (1,1) (0,4) (8,0) (16,1)
    1, 3, 5, 27  (odd sizes)            1     1     1     1     1     1     1
    4, 12, 116   (units 1, 3, 29)       4     4     4     1     4     4     1
    8, 24, 120   (units 1, 3, 15)       8     8     4     1     4     8     1
    16, 48       (units 1, 3)          16     8     4     1     4     8     1

(0,4) narrows through dst alone, (8,0) through src alone, (16,1) pairs a
16-aligned src with an odd dst.  test_gather_rows_matrix_reaches_every_lane_width
checks this table against the rule, and that every width occurs both with one
unit per row and with several.

ogbx_compact_terminals: the `1 << 20` block cap of its launch needs 2.7e8 rows
to cross and is left out.
"""

import ctypes

import numpy as np
import pytest
import torch

from ingest_fixture import FAMILIES, LOAD_KW, expected_load, golden, raw_columns
from ogbench_amd import _lib
from ogbench_amd.datasets import nonzero_positive
from ogbench_amd.utils import (_bind, add_oracle_reps, gather_rows, load_dataset, make_env_and_datasets,
                               relabel_dataset)

pytestmark = pytest.mark.gpu

ROW_BYTES = (1, 3, 4, 5, 8, 12, 16, 24, 27, 48, 116, 120)
OFFSETS = ((0, 0), (8, 8), (4, 4), (1, 1), (0, 4), (8, 0), (16, 1))
GATHER_N = (1, 255, 256, 257)
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def g():
    return golden()


@pytest.fixture(scope='module')
def raw_files(g, tmp_path_factory):
    d = tmp_path_factory.mktemp('ingest')
    paths = {}
    for family in FAMILIES:
        paths[family] = str(d / f'{family}.npz')
        np.savez(paths[family], **raw_columns(g, family))
    return paths


def assert_same_dict(got, exp, what):
    assert list(got) == list(exp), what
    for k, v in exp.items():
        a = got[k].cpu().numpy()
        assert a.dtype == v.dtype and a.shape == v.shape and np.array_equal(a, v), (what, k)


# ---------------------------------------------------------------- load_dataset


@pytest.mark.parametrize('info', [True, False])
@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('family', FAMILIES)
def test_load_dataset_matches_reference(gpu, g, raw_files, family, compact, info):
    """Every family x mode x add_info: key order, dtypes, shapes, values.  The
    1-row file's regular mode gives empty tensors of the right trailing shape."""
    exp = expected_load(g, family, 'compact' if compact else 'regular', info)
    d = load_dataset(raw_files[family], compact_dataset=compact, add_info=info, device=gpu, **LOAD_KW[family])
    assert all(v.device == gpu for v in d.values())
    assert_same_dict(d, exp, (family, compact, info))
    if family == 'one' and not compact:
        assert d['observations'].shape == (0, 29) and d['next_observations'].dtype == torch.float32


@pytest.mark.parametrize('compact', [True, False])
def test_make_env_and_datasets_picks_uint8_and_int32(gpu, g, raw_files, tmp_path, compact):
    """utils.py:209-210: uint8 observations for visual-* and powderworld-*, int32
    actions for powderworld-*.  dataset_only=True: no env is built (a visual-*
    env cannot be made here), the name alone decides the dtypes."""
    mode = 'compact' if compact else 'regular'
    for family, name in (('powder', 'powderworld-easy-play-v0'), ('visual', 'visual-antmaze-large-navigate-v0')):
        raw = raw_columns(g, family)
        np.savez(str(tmp_path / f'{name}.npz'), **raw)
        np.savez(str(tmp_path / f'{name}-val.npz'), **raw)
        train, val = make_env_and_datasets(name, dataset_dir=str(tmp_path), compact_dataset=compact,
                                           dataset_only=True, device=gpu)
        exp = expected_load(g, family, mode, False)
        assert train['observations'].dtype == torch.uint8
        assert train['actions'].dtype == (torch.int32 if family == 'powder' else torch.float32)
        assert_same_dict(train, exp, (name, 'train'))
        assert_same_dict(val, exp, (name, 'val'))


# ---------------------------------------------------------------- ogbx_gather_rows


def lane_width(row_bytes, src_off, dst_off):
    """The rule of ogbx_gather_rows for a 256-aligned base."""
    return next(w for w in (16, 8, 4, 1) if row_bytes % w == 0 and (src_off | dst_off) % w == 0)


def test_gather_rows_matrix_reaches_every_lane_width():
    table = {  # the module docstring's table
        (1, 3, 5, 27): (1, 1, 1, 1, 1, 1, 1),
        (4, 12, 116): (4, 4, 4, 1, 4, 4, 1),
        (8, 24, 120): (8, 8, 4, 1, 4, 8, 1),
        (16, 48): (16, 8, 4, 1, 4, 8, 1),
    }
    assert sorted(rb for rbs in table for rb in rbs) == sorted(ROW_BYTES)
    reached = set()
    for rbs, widths in table.items():
        for rb in rbs:
            for off, w in zip(OFFSETS, widths):
                assert lane_width(rb, *off) == w, (rb, off)
                reached.add((w, rb // w > 1))
    assert reached == {(w, many) for w in (16, 8, 4, 1) for many in (False, True)}


def gather_indices(n, nsrc):
    a = np.arange(n, dtype=np.int64)
    return {
        'identity': a,
        'reversed': nsrc - 1 - a,
        'last': np.full(n, nsrc - 1, np.int64),
        'repeats': (a * 7 + 3) % max(1, nsrc // 2),   # a fixed pattern that visits rows more than once
    }


@pytest.mark.parametrize('row_bytes', ROW_BYTES)
def test_gather_rows_width_and_alignment(gpu, row_bytes):
    """ogbx_gather_rows through ctypes: src and dst at byte offsets inside one
    uint8 allocation, 64 sentinel bytes (and more) on each side of dst.  The
    whole allocation is compared afterwards, so a lane that is too wide, a
    wrong f / units split or a write into src shows up as a difference."""
    L = _bind()
    stream = _lib.stream_of(gpu)
    rng = np.random.RandomState(row_bytes)
    for n in GATHER_N:
        nsrc = n + 3
        for src_off, dst_off in OFFSETS:
            src_end = src_off + nsrc * row_bytes
            dst_at = (src_end + 255) // 256 * 256 + 64 + dst_off
            dst_end = dst_at + n * row_bytes
            host = np.full(dst_end + 64, SENTINEL, np.uint8)
            host[src_off:src_end] = rng.randint(0, 256, nsrc * row_bytes)
            rows = host[src_off:src_end].reshape(nsrc, row_bytes)
            for name, idx in gather_indices(n, nsrc).items():
                assert idx.min() >= 0 and idx.max() < nsrc     # never an index outside src
                buf = torch.from_numpy(host).to(gpu)
                assert buf.data_ptr() % 256 == 0
                didx = torch.from_numpy(idx).to(gpu)
                st = L.ogbx_gather_rows(ctypes.c_void_p(buf.data_ptr() + src_off), row_bytes, _lib.ptr(didx), n,
                                        ctypes.c_void_p(buf.data_ptr() + dst_at), stream)
                assert st == 0
                exp = host.copy()
                exp[dst_at:dst_end] = rows[idx].reshape(-1)     # NumPy fancy indexing on the host copy
                got = buf.cpu().numpy()
                assert np.array_equal(got, exp), (row_bytes, n, (src_off, dst_off), name,
                                                  lane_width(row_bytes, src_off, dst_off))


def test_gather_rows_empty_selection(gpu):
    """n = 0 is a no-op, with the NULL pointers that empty tensors have."""
    src = torch.arange(12, dtype=torch.float32, device=gpu).view(4, 3)
    out = gather_rows(src, torch.empty(0, dtype=torch.int64, device=gpu))
    assert out.shape == (0, 3) and out.dtype == torch.float32
    assert _bind().ogbx_gather_rows(_lib.ptr(src), 12, None, 0, None, _lib.stream_of(gpu)) == 0


def test_gather_rows_grid_stride(gpu):
    """17-byte rows x 1,000,000 = 17,000,000 byte units, above the 16,777,216
    units that the capped launch (65,536 blocks of 256) covers in one trip, so
    the tail is only written by the grid-stride loop.  The wider lanes share
    the loop with the byte lanes."""
    n, rb = 1_000_000, 17
    assert n * rb > 65536 * 256
    src = torch.randint(0, 256, (n, rb), dtype=torch.uint8, generator=torch.Generator().manual_seed(17))
    idx = (torch.arange(n, dtype=torch.int64) * 7919) % n     # 7919 is prime to n: a permutation
    dsrc, didx = src.to(gpu), idx.to(gpu)
    dst = torch.full((n, rb), SENTINEL, dtype=torch.uint8, device=gpu)
    st = _bind().ogbx_gather_rows(_lib.ptr(dsrc), rb, _lib.ptr(didx), n, _lib.ptr(dst), _lib.stream_of(gpu))
    assert st == 0
    assert torch.equal(dst.cpu(), src[idx])


def test_gather_rows_python_wrapper_on_views(gpu):
    """gather_rows makes its source contiguous; a row slice is contiguous
    already and keeps its byte offset, which here breaks the 16-byte alignment
    of the base (24-byte and 20-byte rows), a column slice is copied."""
    gen = torch.Generator().manual_seed(5)
    idx = torch.tensor([4, 0, 0, 255, 17, 254, 3, 3, 128], dtype=torch.int64)
    cases = {
        'f64x3 rows 1:': (torch.rand(257, 3, dtype=torch.float64, generator=gen), lambda s: s[1:]),
        'f32x5 rows 1:': (torch.rand(257, 5, dtype=torch.float32, generator=gen), lambda s: s[1:]),
        'u8x24 rows 3:': (torch.randint(0, 256, (259, 24), dtype=torch.uint8, generator=gen), lambda s: s[3:]),
        'u8x16 cols 3:': (torch.randint(0, 256, (256, 16), dtype=torch.uint8, generator=gen), lambda s: s[:, 3:]),
        'f32x8 cols ::2': (torch.rand(256, 8, dtype=torch.float32, generator=gen), lambda s: s[:, ::2]),
        'i32 1-D 1:': (torch.randint(0, 1 << 30, (257,), dtype=torch.int32, generator=gen), lambda s: s[1:]),
    }
    for name, (src, view) in cases.items():
        d = src.to(gpu)
        assert d.data_ptr() % 16 == 0
        if 'rows' in name:
            assert view(d).is_contiguous() and view(d).data_ptr() % 16 != 0, name
        got = gather_rows(view(d), idx.to(gpu))
        exp = view(src)[idx]
        assert got.dtype == exp.dtype and got.shape == exp.shape and torch.equal(got.cpu(), exp), name
        assert torch.equal(d.cpu(), src), name


# ---------------------------------------------------------------- ogbx_compact_terminals


def layout_terminals(g, n):
    """The fixture's designed layout (row 0 terminal, adjacent terminals,
    lengths 2, 63, 64, 65, ...), repeated to n rows."""
    t = g['raw_ant_terminals']
    return np.tile(t, n // len(t) + 1)[:n].copy()


def compact_reference(t):
    """The reference's lines (ogbench/utils.py:71-73, 89), restated.  NumPy
    concatenates with the Python list [1.0], so the shifted column and the sum
    are float64 and the result is rounded to float32 once.  The sum of two
    float32 is exact in float64, rounding is monotone and 1 is a float32, so
    round(min(exact, 1)) is min(float32 sum, 1): equality with the kernel's
    float32 arithmetic is exact, not approximate."""
    valids = 1.0 - t
    shifted = np.concatenate([t[1:], [1.0]])
    terminals = np.minimum(t + shifted, 1.0).astype(np.float32)
    assert valids.dtype == np.float32 and shifted.dtype == np.float64
    return dict(terminals=terminals, valids=valids, shifted=shifted.astype(np.float32))


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 65537])
def test_compact_terminals_every_output_subset(gpu, g, n):
    L = _bind()
    stream = _lib.stream_of(gpu)
    names = ('terminals', 'valids', 'shifted')                  # the C argument order
    inputs = {
        'layout': layout_terminals(g, n),
        # multiples of 1/8 up to 1.5: min(t + next, 1) clamps some sums and not others, 1 - t goes negative
        'eighths': ((np.arange(n) * 5) % 13 / 8.0).astype(np.float32),
    }
    assert n < 13 or inputs['eighths'].max() == 1.5
    pad = 16
    for tag, t in inputs.items():
        ref = compact_reference(t)
        dt = torch.from_numpy(t).to(gpu)
        for subset in range(1, 8):
            outs = [torch.full((n + pad,), float('nan'), dtype=torch.float32, device=gpu) if subset >> j & 1
                    else None for j in range(3)]
            st = L.ogbx_compact_terminals(_lib.ptr(dt), n, *[_lib.ptr(o) for o in outs], stream)
            assert st == 0
            for name, o in zip(names, outs):
                if o is None:
                    continue
                a = o.cpu().numpy()
                assert np.array_equal(a[:n], ref[name]), (tag, n, subset, name)
                assert np.isnan(a[n:]).all(), (tag, n, subset, name)
            assert np.array_equal(dt.cpu().numpy(), t)


def test_compact_terminals_zero_rows_writes_nothing(gpu):
    t = torch.ones(4, dtype=torch.float32, device=gpu)
    outs = [torch.full((4,), float('nan'), dtype=torch.float32, device=gpu) for _ in range(3)]
    st = _bind().ogbx_compact_terminals(_lib.ptr(t), 0, *[_lib.ptr(o) for o in outs], _lib.stream_of(gpu))
    assert st == 0
    assert all(torch.isnan(o).all().item() for o in outs)


# ---------------------------------------------------------------- relabel


class StubEnv:
    """The attributes relabel_dataset / add_oracle_reps read (maze branch)."""

    def __init__(self, goal, tol):
        self.unwrapped = self
        self._reward_task_id = 1
        self._goal_tol = tol
        self.cur_goal_xy = np.asarray(goal)

    def reset(self):
        return None


def relabel_calls(gpu, qpos, goal, tols):
    """relabel_dataset + add_oracle_reps once per tolerance -> success [K, rows]
    (uint8, after checking rewards = s - 1 and masks = 1 - s) and the reps."""
    rew, msk, reps = [], [], []
    for tol in tols:
        ds = {'qpos': qpos}
        env = StubEnv(goal, float(tol))
        relabel_dataset('antmaze-large-navigate-singletask-task1-v0', env, ds)
        add_oracle_reps('antmaze-large-navigate-oraclerep-v0', env, ds)
        assert ds['rewards'].dtype == torch.float32 and ds['masks'].dtype == torch.float32
        rew.append(ds['rewards'])
        msk.append(ds['masks'])
        reps.append(ds['oracle_reps'])
    rew, msk = torch.stack(rew).cpu().numpy(), torch.stack(msk).cpu().numpy()
    succ = rew + 1.0
    assert set(np.unique(succ)) <= {0.0, 1.0} and np.array_equal(msk, 1.0 - succ)
    return succ.astype(np.uint8), torch.stack(reps).cpu().numpy()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_relabel_on_the_tolerance_boundary(gpu, g, dt):
    """Call k has _goal_tol = the plain float64 distance of row rows[k], which
    therefore sits exactly on `<=`.  For the first 16 rows a distance computed
    with a contracted fma(dx, dx, dy*dy) (either operand order) is an ulp
    larger and fails the row; for the last 16 it is an ulp smaller, and the
    *_below calls (tolerance = that smaller distance) fail the row in the
    reference where a contracted build would pass it."""
    q = g[f'rb_{dt}_qpos']
    rows = g[f'rb_{dt}_rows']
    exp_reps = q if dt == 'f32' else g['rb_f64_reps']
    dq = torch.from_numpy(q.copy()).to(gpu)
    succ, reps = relabel_calls(gpu, dq, g['rb_goal'], g[f'rb_{dt}_tol'])
    assert reps.dtype == np.float32 and all(np.array_equal(r, exp_reps) for r in reps)
    assert all(succ[k, rows[k]] == 1 for k in range(32))
    bad = [k for k in range(32) if not np.array_equal(succ[k], g[f'rb_{dt}_succ'][k])]
    assert not bad, ('calls that differ from the reference', bad)
    below, _ = relabel_calls(gpu, dq, g['rb_goal'], g[f'rb_{dt}_tol_below'])
    bad = [j for j in range(16) if not np.array_equal(below[j], g[f'rb_{dt}_succ_below'][j])]
    assert not bad, ('below-calls that differ from the reference', bad)


@pytest.mark.parametrize('num_rows', [1, 257])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_relabel_qpos_stride_15(gpu, g, dt, num_rows):
    """The ant family's qpos: 15 columns per row, of which the kernel reads two.
    Its values lie on a 1/256 grid, so the float32 copy is the same numbers."""
    q = g['raw_ant_qpos'][:num_rows].astype(np.float32 if dt == 'f32' else np.float64)
    assert np.array_equal(q.astype(np.float64), g['raw_ant_qpos'][:num_rows])
    succ, reps = relabel_calls(gpu, torch.from_numpy(q).to(gpu), g['ant_relabel_goal'], [g['ant_relabel_tol']])
    assert np.array_equal(succ[0], g['ant_relabel_succ'][:num_rows])
    assert reps.shape == (1, num_rows, 2) and np.array_equal(reps[0], q[:, :2].astype(np.float32))


# ---------------------------------------------------------------- nonzero_positive


@pytest.mark.parametrize('n', [1, 7, 257])
def test_nonzero_positive_special_values(gpu, n):
    """-0.0, 0.0, a positive subnormal, -1, NaN, +inf, -inf against
    np.nonzero(x > 0): only the subnormal and +inf are positive."""
    vals = np.array([-0.0, 0.0, 1e-45, -1.0, np.nan, np.inf, -np.inf], np.float32)
    assert 0 < vals[2] < np.finfo(np.float32).tiny
    xs = [vals[i:i + 1] for i in range(7)] if n == 1 else [np.tile(vals, n // 7 + 1)[s:s + n] for s in (0, 3)]
    for x in xs:
        with np.errstate(invalid='ignore'):
            exp = np.nonzero(x > 0)[0]
        got = nonzero_positive(torch.from_numpy(x.copy()).to(gpu))
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), exp), (n, x[:7])
