"""CPU tests of the restatement of TRL batches over the episode ring
(tests/online_trl_np.py): its closed-form pick select against the compaction of
the snapshot's terminals (tests/trl_np.pick_table) on every step of random
histories, and its batch against the reference's recorded behaviour
(tests/golden/online_trl_golden.npz, built by
tests/golden/make_golden_online_trl.py)."""

import os
import re

import numpy as np
import pytest

import online_np as onp
import online_trl_np as otn
import trl_np as tnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_trl_golden.npz')
EXAMPLE = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))
TABLES = {2: 4, 3: 9, 6: 21, 11: 21, 17: 22}  # pickable rows at each snapshot of the fixture


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _rows(rng, n):
    return dict(observations=rng.normal(size=(n, 2)), actions=rng.normal(size=(n, 2)).astype(np.float32),
                next_observations=rng.normal(size=(n, 2)))


def _check_every_step(N, T, steps, done_of):
    ring = onp.OnlineNp(EXAMPLE, N, T)
    rng = np.random.RandomState(N * 131 + T)
    sizes = set()
    for step in range(steps):
        ring.add(_rows(rng, N), done_of(step))
        exp = tnp.pick_table(ring.snapshot()['terminals'])
        P = otn.table(ring)
        assert P.dtype == np.int64 and P.shape == (N + 1,) and P[0] == 0 and (np.diff(P) >= 0).all()
        assert P[-1] == len(exp), (step, P[-1], len(exp))
        np.testing.assert_array_equal(otn.pick_rows(ring), exp, err_msg=f'step {step}')
        sizes.add(int(P[-1]))
    return sizes


@pytest.mark.parametrize('p', [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
@pytest.mark.parametrize('N,T', [(1, 1), (1, 2), (3, 4), (5, 7), (4, 8), (2, 5), (67, 3), (6, 16)])
def test_select_equals_the_compacted_pick_table(N, T, p):
    """3 T + 2 steps, so every slot is rewritten three times; p = 1 and T = 1
    give an empty table on every step."""
    rng = np.random.RandomState(1000 * N + 10 * T + int(10 * p))
    sizes = _check_every_step(N, T, 3 * T + 2, lambda step: rng.rand(N) < p)
    if p == 1.0 or T == 1:
        assert sizes == {0}
    elif p == 0.0:
        assert max(sizes) == N * (T - 1)


def test_select_with_a_never_done_and_an_always_done_env():
    N, T = 3, 5
    rng = np.random.RandomState(5)

    def done_of(step):
        d = rng.rand(N) < 0.3
        d[0], d[2] = False, True
        return d

    ring = onp.OnlineNp(EXAMPLE, N, T)
    for step in range(3 * T + 2):
        ring.add(_rows(rng, N), done_of(step))
        P = otn.table(ring)
        assert P[1] - P[0] == ring.L - 1 and P[3] - P[2] == 0  # every row but the newest; none
        np.testing.assert_array_equal(otn.pick_rows(ring), tnp.pick_table(ring.snapshot()['terminals']))


def test_ordinals_differ_in_uint32():
    """An env whose ordinals cross 2^31 (int32 wraps to negative) and 2^32."""
    for start in (2 ** 31 - 2, 2 ** 32 - 2):
        N, T = 2, 4
        ring = onp.OnlineNp(EXAMPLE, N, T)
        ring.cur_seq[:] = np.array([start, 0], np.uint32).astype(np.int32)
        rng = np.random.RandomState(1)
        for step in range(3 * T):
            with np.errstate(over='ignore'):
                ring.add(_rows(rng, N), np.array([step % 2 == 1, step % 3 == 0]))
            np.testing.assert_array_equal(otn.pick_rows(ring), tnp.pick_table(ring.snapshot()['terminals']))


def _replay(gold, upto):
    ring = onp.OnlineNp(EXAMPLE, 5, 6)
    for t in range(upto):
        ring.add({k: gold[f'hist_{k}'][t] for k in EXAMPLE}, gold['done'][t])
    return ring


@pytest.mark.parametrize('S', list(TABLES))
def test_restatement_reproduces_the_reference(gold, S):
    assert gold['snap_steps'].tolist() == list(TABLES)
    ring = _replay(gold, S)
    P = otn.table(ring)
    assert P[-1] == TABLES[S] == int(gold[f's{S}_pickable'])
    assert (np.diff(P) == 0).any() == (S == 2)  # an env without a pickable row
    for cname, cfg in otn.CONFIGS.items():
        data, draws, exp, keys = tnp.fixture_case(gold, f's{S}_{cname}')
        snap = ring.snapshot()
        assert sorted(snap) == sorted(data)
        for k, v in snap.items():
            assert v.dtype == data[k].dtype
            np.testing.assert_array_equal(v, data[k], err_msg=k)
        out, ix = otn.batch(ring, cfg, draws)
        assert list(out) == [k for k in keys if k != 'terminals']  # the snapshot's own column
        assert set(exp) == set(keys)
        for k, v in out.items():
            assert v.dtype == exp[k].dtype and v.shape == exp[k].shape, k
            np.testing.assert_array_equal(v, exp[k], err_msg=f'{cname} {k}')
        # the reference's idxs are the closed-form select of its picks
        np.testing.assert_array_equal(otn.select(ring, P, draws['pick']), ix['idxs'])
        assert (ix['idxs'] <= ix['mid']).all() and (ix['mid'] < ix['vg']).all()


def test_header_and_source_are_wired_into_the_build():
    mk = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert 'online_trl.hip' in mk and mk.count('ogbx_online_trl.h') == 2  # the header comment and HDRS
    hdr = open(os.path.join(ROOT, 'include', 'ogbx_online_trl.h')).read()
    assert re.search(r'#define\s+OGBX_ONLINE_TRL_API_VERSION\s+1\b', hdr)
    text = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    exports = sorted(set(re.findall(r'\b(ogbx_online_trl_[a-z0-9_]+)\s*\(', text)))
    assert exports == ['ogbx_online_trl_api_version', 'ogbx_online_trl_sample', 'ogbx_online_trl_table',
                       'ogbx_online_trl_table_bytes']
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'ogbx_online_trl.h' in doc and all(f'`{fn}`' in doc for fn in exports)
    from ogbench_amd import _lib, _online_trl

    L = _online_trl.bind()
    assert L is _lib.lib()
    for fn in exports:
        assert hasattr(L, fn) and getattr(L, fn).argtypes is not None, fn
    assert L.ogbx_online_trl_api_version() == _online_trl.ONLINE_TRL_API_VERSION == 1
    tile = int(re.search(r'#define\s+OGBX_ONLINE_TRL_TABLE_TILE\s+(\d+)', hdr).group(1))
    assert tile == _online_trl.ONLINE_TRL_TABLE_TILE
