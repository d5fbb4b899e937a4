"""CPU checks of the visual batch semantics and of the ogbx_visual.h boundary:
the NumPy restatement (tests/visual_np.py) reproduces every array the
reference recorded (tests/golden/visual_golden.npz), libogbx.so exports every
symbol of include/ogbx_visual.h, and its argument checks run before any device
call."""

import ctypes
import os
import re

import numpy as np
import pytest

import visual_np as vnp
from oracle import gcdataset_np as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'visual_golden.npz')
HEADER = os.path.join(ROOT, 'include', 'ogbx_visual.h')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def visual_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(ogbx_visual_[a-z0-9_]+)\s*\(', text)))


@pytest.mark.parametrize('case', list(vnp.CASES))
def test_restatement_reproduces_fixture(gold, case):
    cfg, hgc, evaluation = vnp.CASES[case]
    data, draws, exp = vnp.fixture_case(gold, case)
    crop_from = draws.pop('crop_from', None)
    assert (crop_from is None) == evaluation
    R = len(data['observations'])
    if hgc:
        plain, ix = orc.hgc_sample(data, cfg, draws)
        sel = vnp.hgc_selectors(ix['idxs'], ix['hvg'], ix['hag'], ix['lvg'], vnp.traj_end(data['terminals']), R,
                                *vnp.hgc_steps(cfg))
    else:
        plain, idxs, vg, ag = orc.sample(data, cfg, draws)
        sel = vnp.gc_selectors(idxs, vg, ag, R)
    vis = vnp.visual_batch(data, sel, cfg['frame_stack'], crop_from, hgc=hgc)
    assert set(exp) == set(plain)
    assert len(vis) >= 4
    for k, v in exp.items():
        got = vis[k] if k in vis else plain[k]
        assert got.dtype == v.dtype and got.shape == v.shape, k
        assert np.array_equal(got, v), k
    if crop_from is not None:
        assert crop_from.min() >= 0 and crop_from.max() <= 2 * vnp.PADDING


def test_fixture_covers_short_trajectories_and_every_stack_depth(gold):
    """Case A samples rows whose stack is cut at the trajectory start by 0, 1
    and 2 frames, and its crops move the window (otherwise the fixture would
    not tell a stack or a crop from a copy)."""
    cfg, _, _ = vnp.CASES['A']
    data, draws, exp = vnp.fixture_case(gold, 'A')
    crop_from = draws.pop('crop_from')
    _, idxs, _, _ = orc.sample(data, cfg, draws)
    rows = vnp.stack_rows(idxs, vnp.traj_end(data['terminals']), 3)
    depth = {len(set(r)) for r in rows.tolist()}
    assert depth == {1, 2, 3}
    assert len({tuple(c) for c in crop_from.tolist()}) > 20
    plain = data['observations'][idxs]
    assert not np.array_equal(exp['observations'][..., -2:], plain)


def test_visual_symbols_exported_and_versioned():
    from ogbench_amd import _lib

    L = _lib.lib()
    syms = visual_symbols()
    assert syms == ['ogbx_visual_api_version', 'ogbx_visual_gather']
    assert [s for s in syms if not hasattr(L, s)] == []
    L.ogbx_visual_api_version.restype = ctypes.c_int32
    assert L.ogbx_visual_api_version() == 1
    assert int(re.search(r'#define\s+OGBX_VISUAL_API_VERSION\s+(\d+)', open(HEADER).read()).group(1)) == 1
    # the extension is not part of ogbx.h's ABI
    assert not set(syms) & set(_lib.declared_symbols())


def test_integration_documents_visual_symbols():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'ogbx_visual.h' in doc
    assert [s for s in visual_symbols() if s not in doc] == []


def test_argument_checks_precede_device_calls():
    """Null pointers, frame_stack, padding, selector range and missing index
    outputs are refused (OGBX_EINVAL, message in ogbx_last_error) on any host."""
    from ogbench_amd import _lib
    from ogbench_amd import datasets as D

    L = D._bind()
    buf = D.GcBuffer(10, None, 0, 8, None, None, 0, 0, 0)  # pointers are never dereferenced on the host
    idx = D.VisualIndices(8, None, None, None)

    def call(col=None, buf=buf, idx=idx, F=3, pad=3, total=4):
        cols = (D.VisualColumn * 1)(col) if col is not None else None
        st = L.ogbx_visual_gather(buf, None, ctypes.cast(cols, ctypes.c_void_p) if cols is not None else None,
                                  1 if cols is not None else 0, total, idx, F, pad, None, 0, 0, 0, None, None)
        return st, _lib.last_error()

    good = D.VisualColumn(8, 8, 4, 4, 3, 0, 1, 1)
    assert call(good, buf=None)[0] == _lib.OGBX_EINVAL
    assert call(good, idx=None)[0] == _lib.OGBX_EINVAL
    for F in (0, 9):
        st, msg = call(good, F=F)
        assert st == _lib.OGBX_EINVAL and 'frame_stack' in msg
    st, msg = call(good, pad=-1)
    assert st == _lib.OGBX_EINVAL and 'padding' in msg
    st, msg = call(D.VisualColumn(8, 8, 4, 4, 3, 4, 1, 1))  # selector 4 is HGC's
    assert st == _lib.OGBX_EINVAL and 'selector' in msg
    st, msg = call(D.VisualColumn(8, 8, 4, 4, 3, 2, 1, 1))  # needs value_goal_idxs
    assert st == _lib.OGBX_EINVAL and 'missing index' in msg
    assert call(D.VisualColumn(None, 8, 4, 4, 3, 0, 1, 1))[0] == _lib.OGBX_EINVAL
    assert call(D.VisualColumn(8, 8, 0, 4, 3, 0, 1, 1))[0] == _lib.OGBX_EINVAL
    assert call(good, total=0)[0] == _lib.OGBX_EINVAL
