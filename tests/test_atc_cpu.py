"""CPU checks of the ATC batch semantics and of the ogbx_atc.h boundary: the
NumPy restatement (tests/atc_np.py) reproduces every array the reference
recorded (tests/golden/atc_golden.npz), libogbx.so exports every symbol of
include/ogbx_atc.h, and its argument checks run before any device call."""

import ctypes
import os
import re

import numpy as np
import pytest

import atc_np as anp
import visual_np as vnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'atc_golden.npz')
HEADER = os.path.join(ROOT, 'include', 'ogbx_atc.h')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def atc_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(ogbx_atc_[a-z0-9_]+)\s*\(', text)))


@pytest.mark.parametrize('case', list(anp.CASES))
def test_restatement_reproduces_fixture(gold, case):
    cfg, k = anp.CASES[case]
    data, gk, valid, idxs, draws, exp, keys = anp.fixture_case(gold, case)
    assert gk == k and len(draws['pick']) == 64
    got_valid = anp.valid_idxs(data, k)
    assert got_valid.dtype == valid.dtype and np.array_equal(got_valid, valid)
    crop_from = draws.get('crop_from')
    assert (crop_from is None) == (cfg['p_aug'] is None)
    out, got_idxs = anp.batch(data, cfg, k, draws, crop_from)
    assert np.array_equal(got_idxs, idxs)
    assert list(out) == keys == list(anp.KEYS)
    assert set(exp) == set(keys)
    for key, v in exp.items():
        assert out[key].dtype == v.dtype and out[key].shape == v.shape, key
        assert np.array_equal(out[key], v), key
    if crop_from is not None:
        p = cfg.get('augment_padding', anp.PADDING)
        assert crop_from.shape == (64, 2) and crop_from.min() >= 0 and crop_from.max() <= 2 * p


def test_no_valid_rows_raise_as_the_reference(gold):
    """k = 30 exceeds every trajectory of the fixture (the longest has 30 rows)."""
    data = anp.fixture_case(gold, 'vis')[0]
    assert len(anp.valid_idxs(data, 29)) == 1 and len(anp.valid_idxs(data, 30)) == 0
    with pytest.raises(ValueError, match=r'^No valid ATC indices found for k=30\.$'):
        anp.batch(data, anp.CASES['vis'][0], 30, dict(pick=np.zeros(64, np.int64)))


def test_fixture_exercises_stack_cuts_clamps_and_the_last_row(gold):
    """Otherwise the fixture would not tell a stack or a crop from a copy."""
    cfg, k = anp.CASES['vis']
    data, _, valid, idxs, draws, exp, _ = anp.fixture_case(gold, 'vis')
    tend = vnp.traj_end(data['terminals'])
    for rows in (idxs, idxs + k):
        depth = {len(set(r)) for r in vnp.stack_rows(rows, tend, 3).tolist()}
        assert depth == {1, 2, 3} or (rows is not idxs and depth == {3})
    assert (tend[idxs] == tend[idxs + k]).all()
    cf = draws['crop_from']
    # windows shifted by -4 .. 4 on a 6 x 5 image: the low and the high clamp of both axes
    assert cf.min(0).tolist() == [0, 0] and cf.max(0).tolist() == [8, 8]
    assert len({tuple(c) for c in cf.tolist()}) > 20
    assert not np.array_equal(exp['observations'][..., -2:], data['observations'][idxs])
    # the uncropped state case drew its offsets all the same
    assert 'crop_from' in anp.fixture_case(gold, 'stack_state')[4]
    # k_last: the anchor's stack clamps to itself, the positive is the trajectory's last row
    data, k, valid, idxs, _, exp, _ = anp.fixture_case(gold, 'k_last')
    assert len(valid) == 1 and (idxs == valid[0]).all() and tend[valid[0]] == valid[0] + 29
    frame = data['observations'][valid[0]]
    assert np.array_equal(exp['observations'][0], np.concatenate([frame] * 3, -1))
    assert np.array_equal(exp['positive_observations'][0][..., -2:], data['observations'][tend[valid[0]]])


def test_atc_symbols_exported_and_versioned():
    from ogbench_amd import _lib

    L = _lib.lib()
    syms = atc_symbols()
    assert syms == ['ogbx_atc_api_version', 'ogbx_atc_sample', 'ogbx_atc_valid_idxs']
    assert [s for s in syms if not hasattr(L, s)] == []
    L.ogbx_atc_api_version.restype = ctypes.c_int32
    assert L.ogbx_atc_api_version() == 1
    assert int(re.search(r'#define\s+OGBX_ATC_API_VERSION\s+(\d+)', open(HEADER).read()).group(1)) == 1
    # the extension is not part of ogbx.h's ABI
    assert not set(syms) & set(_lib.declared_symbols())


def test_integration_documents_atc_symbols():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'ogbx_atc.h' in doc
    assert [s for s in atc_symbols() if s not in doc] == []


def test_design_quotes_the_sampler_record():
    """Every figure of DESIGN 4.9's table is the record's (profiles/atc_sampler.json),
    formatted as the document prints it, and both recorded conditions hold."""
    import json

    with open(os.path.join(ROOT, 'profiles', 'atc_sampler.json')) as f:
        rec = json.load(f)
    with open(os.path.join(ROOT, 'DESIGN.md'), encoding='utf-8') as f:
        body = ' '.join(f.read().split())
    v = rec['variants']

    def cell(x):
        return f"{x['median_us']:.1f} ({x['spread_us']:.1f})"

    for name in ('atc', 'composed', 'vis_b', 'vis_b_parent'):
        want = f"| {cell(v[name]['new'])} | {cell(v[name]['refill'])} |"
        assert want in body, (name, want)
    assert f"| {cell(v['copy'])} | |" in body
    for name, cond in rec['conditions'].items():
        for style in ('new', 'refill'):
            assert cond[style]['holds'] is True, (name, style)
    assert all(len(v[name][style]['windows_us']) >= rec['windows'] for name in ('atc', 'composed', 'vis_b')
               for style in ('new', 'refill'))


def test_package_exports_the_sampler():
    import ogbench_amd
    from ogbench_amd import datasets as D

    assert ogbench_amd.ATCDataset is D.ATCDataset and 'ATCDataset' in ogbench_amd.__all__


def test_argument_checks_precede_device_calls():
    """Null pointers, sizes, k, frame_stack, padding, a missing or empty
    valid(k) and images that cannot be staged are refused (OGBX_EINVAL, message
    in ogbx_last_error) on any host."""
    from ogbench_amd import _lib
    from ogbench_amd import datasets as D

    L = D._bind()
    buf = D.GcBuffer(10, None, 0, 8, None, None, 0, 0, 0)  # pointers are never dereferenced on the host
    periodic = D.GcBuffer(10, None, 0, 8, None, None, 5, 5, 4)
    good = D.AtcColumn(8, 8, 8, 4, 4, 3, 1)

    def call(col=good, buf=buf, total=4, k=1, valid=8, n=3, F=3, pad=4, idxs=None, outs=None):
        st = L.ogbx_atc_sample(buf, col, total, k, valid, n, F, pad, idxs, None, None, 0, 0, 0, outs, None)
        return st, _lib.last_error()

    assert call(buf=None)[0] == _lib.OGBX_EINVAL
    assert call(col=None)[0] == _lib.OGBX_EINVAL
    assert call(buf=D.GcBuffer(10, None, 0, None, None, None, 0, 0, 0))[0] == _lib.OGBX_EINVAL
    for col in (D.AtcColumn(None, 8, 8, 4, 4, 3, 1), D.AtcColumn(8, None, 8, 4, 4, 3, 1),
                D.AtcColumn(8, 8, None, 4, 4, 3, 1), D.AtcColumn(8, 8, 8, 0, 4, 3, 1),
                D.AtcColumn(8, 8, 8, 4, 4, 0, 1)):
        assert call(col=col)[0] == _lib.OGBX_EINVAL
    st, msg = call(total=0)
    assert st == _lib.OGBX_EINVAL and 'total' in msg
    st, msg = call(k=-1)
    assert st == _lib.OGBX_EINVAL and 'k must be' in msg
    for F in (0, 9):
        st, msg = call(F=F)
        assert st == _lib.OGBX_EINVAL and 'frame_stack' in msg
    st, msg = call(pad=-1)
    assert st == _lib.OGBX_EINVAL and 'padding' in msg
    st, msg = call(valid=None)  # no table, not periodic, no explicit idxs
    assert st == _lib.OGBX_EINVAL and 'table' in msg
    st, msg = call(n=0)
    assert st == _lib.OGBX_EINVAL and 'empty' in msg
    st, msg = call(valid=None, buf=periodic, k=5)  # no row of a 5-row trajectory has a fifth successor
    assert st == _lib.OGBX_EINVAL and 'empty' in msg
    st, msg = call(outs=D.AtcOutputs(None, None, 8, None))
    assert st == _lib.OGBX_EINVAL and 'crop' in msg
    st, msg = call(col=D.AtcColumn(8, 8, 8, 1 << 15, 1 << 15, 4, 1))
    assert st == _lib.OGBX_EINVAL and 'too large' in msg
    st, msg = call(col=D.AtcColumn(8, 8, 8, 2, 1 << 14, 3, 1), F=2)  # a 48-KB row, 32 KB of LDS per frame
    assert st == _lib.OGBX_EINVAL and 'too wide' in msg
    # ogbx_atc_valid_idxs
    out = ctypes.c_void_p(8)
    assert L.ogbx_atc_valid_idxs(None, 1, out, out, None) == _lib.OGBX_EINVAL
    assert L.ogbx_atc_valid_idxs(buf, 1, None, out, None) == _lib.OGBX_EINVAL
    assert L.ogbx_atc_valid_idxs(buf, 1, out, None, None) == _lib.OGBX_EINVAL
    assert L.ogbx_atc_valid_idxs(buf, -1, out, out, None) == _lib.OGBX_EINVAL
    assert 'k must be' in _lib.last_error()
