"""CPU: the ingest fixture (tests/golden/ingest_golden.npz, written by
tests/golden/make_golden_ingest.py from the reference's load_dataset /
relabel_dataset / add_oracle_reps) holds what its generator promised, and the
NumPy oracle's load_dataset (oracle/gcdataset_np.py, which every GC test
builds its data with) reproduces it."""

import os

import numpy as np
import pytest

from ingest_fixture import LOAD_KW, PATH as G, expected_load, golden, raw_columns
from oracle import gcdataset_np as gco

INFO = ('qpos', 'qvel', 'button_states')
ROWS = {'ant': 263, 'visual': 263, 'powder': 257, 'one': 1}
LENGTHS = {'ant': [1, 1, 1, 2, 63, 64, 65, 62, 4], 'visual': [1, 1, 1, 2, 63, 64, 65, 62],
           'powder': [1, 1, 1, 2, 63, 64, 65, 60], 'one': [1]}
TAIL = {'ant': 0, 'visual': 4, 'powder': 0, 'one': 0}
RAW_SPEC = {
    'ant': dict(observations=('float32', (29,)), actions=('float32', (8,)), terminals=('float32', ()),
                qpos=('float64', (15,)), qvel=('float64', (14,)), button_states=('uint8', (5,))),
    'visual': dict(observations=('uint8', (4, 4, 3)), actions=('float32', (2,)), terminals=('float32', ())),
    'powder': dict(observations=('uint8', (3, 3, 3)), actions=('int32', ()), terminals=('float32', ())),
}
RAW_SPEC['one'] = RAW_SPEC['ant']


@pytest.fixture(scope='module')
def g():
    return golden()


def test_fixture_file_is_small_and_plain():
    assert os.path.getsize(G) <= 300_000
    with np.load(G, allow_pickle=False) as f:
        assert all(f[k].dtype.kind in 'fiuU' for k in f.files)


@pytest.mark.parametrize('family', ['ant', 'visual', 'powder', 'one'])
def test_fixture_raw_columns_and_terminal_layout(g, family):
    n = ROWS[family]
    spec = RAW_SPEC[family]
    assert sorted(raw_columns(g, family)) == sorted(spec)
    for k, (dtype, trail) in spec.items():
        v = g[f'raw_{family}_{k}']
        assert v.dtype.name == dtype and v.shape == (n,) + trail, (family, k)
    assert n % 64 != 0 and n % 256 != 0
    t = g[f'raw_{family}_terminals']
    assert set(np.unique(t)) <= {0.0, 1.0}
    locs = np.nonzero(t)[0]
    assert np.diff(np.concatenate([[-1], locs])).tolist() == LENGTHS[family]
    assert n - 1 - locs[-1] == TAIL[family]
    assert t[0] == 1                                          # a terminal at row 0
    if family != 'one':
        assert t[:3].tolist() == [1, 1, 1]                    # adjacent terminals: length-1 trajectories
        assert locs[6] + 1 < 256 <= locs[7]                   # one trajectory runs across row 256
        assert (t[-1] == 1) == (family != 'visual')


@pytest.mark.parametrize('family', ['ant', 'visual', 'powder', 'one'])
def test_fixture_loads_have_the_promised_keys(g, family):
    info_keys = [k for k in INFO if k in RAW_SPEC[family]]
    base = ['observations', 'actions', 'terminals']
    n = ROWS[family]
    t = g[f'raw_{family}_terminals']
    kept = int((t == 0).sum())
    for mode, last in (('compact', 'valids'), ('regular', 'next_observations')):
        for info in (True, False):
            d = expected_load(g, family, mode, info)
            assert list(d) == base + (info_keys if info else []) + [last], (family, mode, info)
            for k, v in d.items():
                dtype, trail = RAW_SPEC[family]['observations' if k == 'next_observations' else
                                                'terminals' if k == 'valids' else k]
                rows = n if mode == 'compact' else kept - (k == 'next_observations' and family == 'visual')
                assert v.dtype.name == dtype and v.shape == (rows,) + trail, (family, mode, k)
    # compact stores only what differs from the raw columns
    stored = sorted(k for k in g if k.startswith(f'exp_{family}_compact_'))
    want = ['terminals', 'valids'] if family != 'one' else ['valids']
    assert stored == [f'exp_{family}_compact_{k}' for k in want]
    if family == 'visual':  # the reference's regular mode: one more observation than next_observation
        assert len(g['exp_visual_regular_observations']) == len(g['exp_visual_regular_next_observations']) + 1
    if family == 'one':
        assert g['exp_one_regular_observations'].shape == (0, 29)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_fixture_relabel_boundary_block(g, dt):
    q = g[f'rb_{dt}_qpos']
    rows, tol, succ = g[f'rb_{dt}_rows'], g[f'rb_{dt}_tol'], g[f'rb_{dt}_succ']
    tol_b, succ_b = g[f'rb_{dt}_tol_below'], g[f'rb_{dt}_succ_below']
    assert q.dtype == (np.float32 if dt == 'f32' else np.float64) and q.shape == (2048, 2)
    assert rows.shape == (32,) and len(set(rows.tolist())) == 32 and tol.shape == (32,) and tol.dtype == np.float64
    assert succ.dtype == np.uint8 and succ.shape == (32, 2048) and set(np.unique(succ)) == {0, 1}
    assert succ_b.dtype == np.uint8 and succ_b.shape == (16, 2048) and tol_b.shape == (16,)
    goal = g['rb_goal']
    assert goal.tolist() == [12.3, -4.7]
    d = np.linalg.norm(q.astype(np.float64) - goal, axis=-1)
    assert np.array_equal(tol, d[rows])                       # row k sits exactly on <=
    assert np.array_equal(succ, (d[None, :] <= tol[:, None]).astype(np.uint8))
    assert np.array_equal(succ_b, (d[None, :] <= tol_b[:, None]).astype(np.uint8))
    for k in range(32):
        assert succ[k, rows[k]] == 1 and 0 < succ[k].sum() < 2048
        assert (d < tol[k]).sum() < succ[k].sum()             # `<` written for `<=` loses row k
    for j in range(16):
        r = rows[16 + j]
        assert tol_b[j] < tol[16 + j] and np.nextafter(tol_b[j], np.inf) == tol[16 + j]
        assert succ_b[j, r] == 0 and 0 < succ_b[j].sum() < 2048


def test_fixture_ant_relabel(g):
    s = g['ant_relabel_succ']
    assert s.dtype == np.uint8 and s.shape == (263,) and 20 < s.sum() < 243
    d = np.linalg.norm(g['raw_ant_qpos'][:, :2] - g['ant_relabel_goal'], axis=-1)
    assert np.array_equal(s, (d <= float(g['ant_relabel_tol'])).astype(np.uint8))


@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('family', ['ant', 'visual', 'powder'])
def test_oracle_load_dataset_matches_reference(g, family, compact):
    raw = raw_columns(g, family)
    exp = expected_load(g, family, 'compact' if compact else 'regular', True)
    got = gco.load_dataset(raw, compact_dataset=compact, add_info=True, **LOAD_KW[family])
    assert list(got) == list(exp)
    for k, v in exp.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v), (family, k)
