"""GPU: the samplers' shared row gather (copy_tile / copy_rows of
csrc/gc_device.h) at its width, stride, tile and table edges, through
ogbx_replay_sample, ogbx_gc_sample, ogbx_hgc_sample, the look-ahead kernels and
the sampler plans.

A pure gather check, independent of the draw chain (which the parity suites
pin): every column's source and destination lie at chosen byte offsets inside
one uint8 allocation whose base is asserted 256-aligned, with 64 sentinel bytes
and more on both sides of every destination, and after the call the WHOLE
allocation must equal the host expectation -- destination rows = source[sel],
everything else untouched -- where sel comes from the indices the kernel itself
reports (next = min(idx + 1, R - 1); the remaining HGC selectors from the NumPy
restatement of high_next in tests/visual_np.py).  All comparisons are bit-exact.

Which branch a case takes cannot be observed from outside; the tables are those
of tests/gather_np.py, and tests/test_gather_cpu.py proves that they reach
every copy unit, the flat and the tiled path, three and four copying waves, one
and several trips of the job loop and both table sizes.  Every index handed to
the library lies inside its source.

Out of scope: the trl, online* and ring samplers reach copy_tile with the same
template arguments and the same `tile <= 4 && flat4` rule.
"""

import ctypes
import types

import numpy as np
import pytest
import torch

import gather_np as G
import visual_np
from ogbench_amd import _lib
from ogbench_amd import datasets as D
from oracle import gcdataset_np as orc
from test_oracle_gc import CONFIGS
from test_oracle_hgc import HGC_CONFIGS

pytestmark = pytest.mark.gpu

LENGTHS = (5, 17, 64, 3, 40, 31, 32)     # ragged trajectories, 192 rows
SEED = 77


@pytest.fixture(scope='module')
def w(gpu):
    """A small trajectory buffer (compact layout) and its GC / HGC samplers:
    the library's own _buf / _cfg, used with test-owned column tables."""
    R = sum(LENGTHS)
    term = np.zeros(R, np.float32)
    term[np.cumsum(LENGTHS) - 1] = 1
    rng = np.random.RandomState(0)
    raw = dict(observations=rng.normal(size=(R, 2)).astype(np.float32),
               actions=rng.normal(size=(R, 1)).astype(np.float32), terminals=term)
    data = orc.load_dataset(raw, compact_dataset=True)
    ds = D.Dataset(data, device=gpu)
    gc = D.GCDataset(ds, dict(CONFIGS['gciql'], p_aug=None, frame_stack=None, lookahead=False), seed=SEED)
    hgc = D.HGCDataset(ds, dict(HGC_CONFIGS['hlow'], p_aug=None, lookahead=False), seed=SEED)
    assert gc.size == R and gc.period == (0, 0, 0)
    return types.SimpleNamespace(gpu=gpu, R=R, gc=gc, hgc=hgc, L=hgc._Lh, stream=_lib.stream_of(gpu),
                                 tend=gc.traj_end.cpu().numpy())


class Image:
    """The byte image of a column table on the device, and its descriptors."""

    def __init__(self, w, cols, total, seed, num_rows=None):
        self.cols, self.total, self.R = cols, total, num_rows or w.R
        self.host, self.at = G.layout(cols, self.R, total, seed)
        self.pristine = torch.from_numpy(self.host).to(w.gpu)
        self.dev = self.pristine.clone()
        base = self.dev.data_ptr()
        assert base % 256 == 0 and self.pristine.data_ptr() % 256 == 0
        self.arr = (D.GcColumn * len(cols))(*[
            D.GcColumn(base + s, base + d, c['row_bytes'], c['select'], c['stride'])
            for c, (s, d, _) in zip(cols, self.at)])
        self.ptr = ctypes.cast(self.arr, ctypes.c_void_p)

    def reset(self):
        self.dev.copy_(self.pristine)

    def check(self, sels, what):
        exp = G.expected_image(self.host, self.cols, self.at, sels, self.R, self.total)
        got = self.dev.cpu().numpy()
        if not np.array_equal(got, exp):
            i = int(np.nonzero(got != exp)[0][0])
            where = [(k, c, 'dst' if d - G.GUARD <= i else 'src') for k, (c, (s, d, p)) in
                     enumerate(zip(self.cols, self.at)) if s <= i < s + self.R * p or d - G.GUARD <= i <
                     d + self.total * c['row_bytes'] + G.GUARD]
            raise AssertionError((what, 'first differing byte', i, 'of', len(exp), where,
                                  int((got != exp).sum()), 'bytes differ'))


def i64(w, n, fill=-1):
    return torch.full((n,), fill, dtype=torch.int64, device=w.gpu)


def f64(w, n):
    return torch.full((n,), float('nan'), dtype=torch.float64, device=w.gpu)


def gc_outputs(w, n):
    return dict(idxs=i64(w, n), vg=i64(w, n), ag=i64(w, n), masks=f64(w, n), rewards=f64(w, n))


def gc_sels(w, o):
    idx, vg, ag = (o[k].cpu().numpy() for k in ('idxs', 'vg', 'ag'))
    return visual_np.gc_selectors(idx, vg, ag, w.R)


def gc_direct(w, im, idxs=None, seed=SEED, call=0):
    o = gc_outputs(w, im.total)
    dr = D.GcDraws(idxs=idxs.data_ptr()) if idxs is not None else None
    _lib.check(w.L.ogbx_gc_sample(w.gc._buf, w.gc._cfg, im.ptr, len(im.cols), im.total, 1, dr, seed, call,
                                  _lib.ptr(o['idxs']), _lib.ptr(o['vg']), _lib.ptr(o['ag']), _lib.ptr(o['masks']),
                                  _lib.ptr(o['rewards']), None, w.stream))
    return o


def hgc_outputs(w, n):
    o = {k: (f64(w, n) if k.endswith(('masks', 'rewards')) else i64(w, n)) for k in D._HGC_SCALARS}
    return o, D.HgcOutputs(*[o[k].data_ptr() for k in D._HGC_SCALARS])


def hgc_sels(w, o):
    idx, hvg, hag, lvg = (o[k].cpu().numpy() for k in D._HGC_SCALARS[:4])
    h = w.hgc
    return visual_np.hgc_selectors(idx, hvg, hag, lvg, w.tend, w.R, h.value_subgoal_steps, h.low_subgoal_steps,
                                   h.actor_subgoal_steps)


def hgc_direct(w, im, idxs=None, seed=SEED, call=0):
    o, outs = hgc_outputs(w, im.total)
    dr = None
    if idxs is not None:
        dr = D.HgcDraws()
        dr.gc.idxs = idxs.data_ptr()
    _lib.check(w.L.ogbx_hgc_sample(w.hgc._buf, w.hgc._cfg, w.hgc._hcfg, im.ptr, len(im.cols), im.total, 1, dr, seed,
                                   call, outs, None, w.stream))
    return o


def same_outputs(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), (what, k)


def dev_idxs(w, idx):
    assert idx.min() >= 0 and idx.max() < w.R     # never a row outside the sources
    return torch.from_numpy(idx).to(w.gpu)


# ---------------------------------------------------------------- width x alignment x stride


@pytest.mark.parametrize('row_bytes', G.ROW_BYTES)
def test_width_alignment_and_stride(w, row_bytes):
    """Every (src, dst) offset pair and source stride of a row size (12 bytes:
    also the packed record), through ogbx_replay_sample with explicit idxs
    (16-entry table, selectors 0-1) and ogbx_gc_sample with injected idxs
    (32-entry table, selectors 0-3), at totals 1, 3, 64 and 257."""
    header = torch.tensor([0, w.R, 0, w.R], dtype=torch.int64, device=w.gpu)     # (pointer, size) x 2: a full ring
    for entry in G.ENTRY_TABLE:
        for ti, cols in enumerate(G.sweep_tables(row_bytes, entry)):
            for total in G.SWEEP_TOTALS:
                im = Image(w, cols, total, seed=row_bytes + ti)
                for name, idx in G.explicit_idxs(total, w.R).items():
                    what = (entry, row_bytes, ti, total, name, G.flat4_tiled(cols, total))
                    didx = dev_idxs(w, idx)
                    im.reset()
                    if entry == 'replay':
                        out = i64(w, total)
                        st = w.L.ogbx_replay_sample(_lib.ptr(header), 0, w.R, im.ptr, len(cols), total,
                                                    _lib.ptr(didx), SEED, 0, _lib.ptr(out), None, w.stream)
                        _lib.check(st)
                        got = out.cpu().numpy()
                        sels = {0: got, 1: np.minimum(got + 1, w.R - 1)}
                    else:
                        o = gc_direct(w, im, idxs=didx)
                        sels = gc_sels(w, o)
                    assert np.array_equal(sels[0], idx), what
                    im.check(sels, what)


# ---------------------------------------------------------------- tile and grid edges


@pytest.mark.parametrize('total', G.EDGE_TOTALS)
def test_tile_and_grid_edges(w, total):
    """ogbx_gc_sample, the injected and the Philox instance, with a table that
    takes the job path below 5120 samples and copy_rows from there on, one
    that a 1-byte column keeps off the job path, and (below the two largest
    totals) one of rows with more units than threads: only a tile of several
    samples makes copy_rows carry from one such row into the next."""
    for name, cols in G.edge_tables(total).items():
        im = Image(w, cols, total, seed=total)
        for inst in ('injected', 'philox'):
            what = (total, name, inst)
            im.reset()
            if inst == 'injected':
                idx = G.explicit_idxs(total, w.R)['repeats_and_last']
                o = gc_direct(w, im, idxs=dev_idxs(w, idx))
                assert np.array_equal(o['idxs'].cpu().numpy(), idx), what
            else:
                o = gc_direct(w, im, call=3)
            im.check(gc_sels(w, o), what)


# ---------------------------------------------------------------- job loop


@pytest.mark.parametrize('num_cols,total', G.JOB_CASES)
def test_job_loop(w, num_cols, total):
    """Flat tables whose num_cols x n_here sits below, on and above a full trip
    of the job loop, at tiles 1 and 4 (ogbx_gc_sample; up to 16 columns also
    through ogbx_replay_sample's 16-entry table)."""
    cols = G.flat_table(num_cols, 4)
    im = Image(w, cols, total, seed=num_cols)
    for inst in ('injected', 'philox'):
        im.reset()
        idx = G.explicit_idxs(total, w.R)['repeats_and_last']
        o = gc_direct(w, im, idxs=dev_idxs(w, idx) if inst == 'injected' else None, call=1)
        im.check(gc_sels(w, o), (num_cols, total, inst))
    if num_cols <= 16:
        cols = G.flat_table(num_cols, 2)
        im = Image(w, cols, total, seed=num_cols + 1)
        header = torch.tensor([0, w.R, 0, w.R], dtype=torch.int64, device=w.gpu)
        out = i64(w, total)
        _lib.check(w.L.ogbx_replay_sample(_lib.ptr(header), 1, w.R, im.ptr, num_cols, total, None, SEED, 2,
                                          _lib.ptr(out), None, w.stream))
        got = out.cpu().numpy()
        im.check({0: got, 1: np.minimum(got + 1, w.R - 1)}, (num_cols, total, 'replay'))


# ---------------------------------------------------------------- look-ahead kernels


def ahead_call(w, kind, im, call, ahead_in, ahead_out):
    if kind == 'gc':
        o = gc_outputs(w, im.total)
        _lib.check(w.L.ogbx_gc_sample_ahead(w.gc._buf, w.gc._cfg, im.ptr, len(im.cols), im.total, 1, SEED, call,
                                            _lib.ptr(ahead_in), _lib.ptr(ahead_out), _lib.ptr(o['idxs']),
                                            _lib.ptr(o['vg']), _lib.ptr(o['ag']), _lib.ptr(o['masks']),
                                            _lib.ptr(o['rewards']), w.stream))
        return o
    o, outs = hgc_outputs(w, im.total)
    _lib.check(w.L.ogbx_hgc_sample_ahead(w.hgc._buf, w.hgc._cfg, w.hgc._hcfg, im.ptr, len(im.cols), im.total, 1, SEED,
                                         call, _lib.ptr(ahead_in), _lib.ptr(ahead_out), outs, w.stream))
    return o


AHEAD_TABLES = ['nonflat'] + [f'flat{n}' for n in G.AHEAD_FLAT_COLS]


@pytest.mark.parametrize('table', AHEAD_TABLES)
@pytest.mark.parametrize('form', list(G.AHEAD_FORMS))
@pytest.mark.parametrize('kind', ['gc', 'hgc'])
def test_lookahead_kernels(w, kind, form, table):
    """ogbx_gc_sample_ahead / ogbx_hgc_sample_ahead: the miss kernel without
    ahead_out (four copying waves) and with it (three), and the hit kernel
    (three waves, per-wave selector column; non-temporal stores for HGC), each
    with a flat and a non-flat table.  Bit-equal to the direct call of the same
    seed and call index, and equal to the pure gather expectation."""
    nsel = 4 if kind == 'gc' else 10
    cols = G.ahead_nonflat_table(nsel) if table == 'nonflat' else G.flat_table(int(table[4:]), nsel)
    words = 8 if kind == 'gc' else 20     # OGBX_GC_AHEAD_WORDS / OGBX_HGC_AHEAD_WORDS
    direct, sels_of = (gc_direct, gc_sels) if kind == 'gc' else (hgc_direct, hgc_sels)
    call = 4
    for total in G.AHEAD_TOTALS:
        what = (kind, form, table, total)
        a, b = Image(w, cols, total, seed=total), Image(w, cols, total, seed=total)
        bufs = [i64(w, total * words, 0) for _ in range(2)]
        if form == 'miss':
            oa = ahead_call(w, kind, a, call, None, None)
        elif form == 'miss_out':
            oa = ahead_call(w, kind, a, call, None, bufs[0])
        else:
            ahead_call(w, kind, a, call - 1, None, bufs[0])     # stores call's selectors
            a.reset()
            oa = ahead_call(w, kind, a, call, bufs[0], bufs[1])
        ob = direct(w, b, call=call)
        same_outputs(oa, ob, what)
        sels = sels_of(w, ob)
        b.check(sels, what + ('direct',))
        a.check(sels, what + ('ahead',))
        assert np.array_equal(a.host, b.host)


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('num_cols', G.PLAN_COLS)
@pytest.mark.parametrize('kind', ['gc', 'hgc'])
def test_sampler_plan_table_sizes(w, kind, num_cols, flat):
    """ogbx_gc_plan_*: 16 columns launch with the 16-entry table, 17 with the
    32-entry one; calls 0, 1, 2 of a stream are a miss and two hits."""
    nsel = 4 if kind == 'gc' else 10
    cols = G.flat_table(num_cols, nsel) if flat else G.flat_table(num_cols - 1, nsel) + [G.col(3, 1, 1, 0, nsel - 1)]
    assert len(cols) == num_cols and G.flat4_table(cols) == flat
    direct, sels_of = (gc_direct, gc_sels) if kind == 'gc' else (hgc_direct, hgc_sels)
    L = w.L
    for total in (5, 1024):
        plan = ctypes.c_void_p()
        hcfg = ctypes.addressof(w.hgc._hcfg) if kind == 'hgc' else None
        host = w.hgc if kind == 'hgc' else w.gc
        _lib.check(L.ogbx_gc_plan_create(host._buf, host._cfg, hcfg, SEED, 1, ctypes.byref(plan)))
        try:
            a, b = Image(w, cols, total, seed=num_cols), Image(w, cols, total, seed=num_cols)
            if kind == 'gc':
                oa = gc_outputs(w, total)
                st = L.ogbx_gc_plan_set_batch(plan, 0, a.ptr, num_cols, total, 1, _lib.ptr(oa['idxs']),
                                              _lib.ptr(oa['vg']), _lib.ptr(oa['ag']), _lib.ptr(oa['masks']),
                                              _lib.ptr(oa['rewards']), None)
            else:
                oa, outs = hgc_outputs(w, total)
                st = L.ogbx_gc_plan_set_batch(plan, 0, a.ptr, num_cols, total, 1, None, None, None, None, None,
                                              ctypes.addressof(outs))
            _lib.check(st)
            assert L.ogbx_gc_plan_hits(plan) == 0
            for call in range(3):
                what = (kind, num_cols, flat, total, call)
                a.reset()
                b.reset()
                _lib.check(L.ogbx_gc_plan_sample(plan, 0, call, w.stream))
                ob = direct(w, b, call=call)
                same_outputs(oa, ob, what)
                sels = sels_of(w, ob)
                b.check(sels, what + ('direct',))
                a.check(sels, what + ('plan',))
                assert L.ogbx_gc_plan_hits(plan) == call, what     # calls 1 and 2 ran the hit kernel
        finally:
            torch.cuda.synchronize()
            _lib.check(L.ogbx_gc_plan_destroy(plan))


# ---------------------------------------------------------------- HGC tiled kernel


@pytest.mark.parametrize('total', G.HGC_TOTALS)
def test_hgc_tiled_kernel_all_selectors(w, total):
    """ogbx_hgc_sample with columns on all ten selectors: the job path (tiles 1
    and 4) and copy_rows (tile 5), injected and Philox instance."""
    for flat in (True, False):
        cols = G.hgc_table(flat)
        im = Image(w, cols, total, seed=total)
        for inst in ('injected', 'philox'):
            im.reset()
            idx = G.explicit_idxs(total, w.R)['repeats_and_last']
            o = hgc_direct(w, im, idxs=dev_idxs(w, idx) if inst == 'injected' else None, call=2)
            if inst == 'injected':
                assert np.array_equal(o['idxs'].cpu().numpy(), idx)
            im.check(hgc_sels(w, o), (total, flat, inst))
