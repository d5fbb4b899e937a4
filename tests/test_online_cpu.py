"""CPU tests of the episode-ring restatement (tests/online_np.py): its tables
against a brute-force model that keeps every env's whole history, and the
sample over its snapshot against the reference's recorded behaviour
(tests/golden/online_golden.npz, built by tests/golden/make_golden_online.py)."""

import os
import re

import numpy as np
import pytest

import online_np as onp
from oracle import gcdataset_np as gco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_golden.npz')
EXAMPLE = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _same(got, exp, what=''):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    np.testing.assert_array_equal(got, exp, err_msg=what)


def _rows(rng, n):
    return dict(observations=rng.normal(size=(n, 2)), actions=rng.normal(size=(n, 2)).astype(np.float32),
                next_observations=rng.normal(size=(n, 2)))


@pytest.mark.parametrize('p', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('T', [1, 2, 5])
@pytest.mark.parametrize('N', [1, 3])
def test_tables_equal_the_brute_force_model(N, T, p):
    """p = 1: an episode every step, so every slot of ep_end is reused."""
    rng = np.random.RandomState(100 * N + 10 * T + int(10 * p))
    ring, brute = onp.OnlineNp(EXAMPLE, N, T), onp.Brute(N, T)
    dtypes = {k: v.dtype for k, v in ring.cols.items()}
    for step in range(4 * T):
        rows, done = _rows(rng, N), rng.rand(N) < p
        written = ring.add(rows, done)
        brute.add(rows, done)
        assert written.tolist() == [(step % T) * N + e for e in range(N)]
        assert ring.S == step + 1 and ring.L == min(step + 1, T)
        got, exp = ring.snapshot(), brute.snapshot(dtypes)
        assert list(got) == list(exp)
        for k in exp:
            _same(got[k], exp[k], f'{k} after step {step}')
        assert got['terminals'][ring.L - 1::ring.L].tolist() == [1.0] * N  # every env's newest row
        # the flat -> physical map is a bijection onto the live rows
        phys = ring.phys(np.arange(N * ring.L))
        assert len(set(phys.tolist())) == N * ring.L and phys.max() < N * T
    if p == 1.0:
        assert ring.cur_seq.tolist() == [4 * T] * N


def test_clear_restarts_the_ordinals():
    rng = np.random.RandomState(3)
    ring = onp.OnlineNp(EXAMPLE, 3, 4)
    for _ in range(6):
        ring.add(_rows(rng, 3), rng.rand(3) < 0.5)
    ring.clear()
    assert ring.S == 0 and ring.cur_seq.tolist() == [0, 0, 0]
    brute = onp.Brute(3, 4)
    for _ in range(3):
        rows, done = _rows(rng, 3), rng.rand(3) < 0.5
        ring.add(rows, done)
        brute.add(rows, done)
    exp = brute.snapshot({k: v.dtype for k, v in ring.cols.items()})
    for k, v in ring.snapshot().items():
        _same(v, exp[k], k)


def _replay(gold, upto):
    ring = onp.OnlineNp(EXAMPLE, 5, 6)
    for t in range(upto):
        ring.add({k: gold[f'in_{k}'][t] for k in EXAMPLE}, gold['done'][t])
    return ring


def test_golden_pattern_has_the_designed_cases(gold):
    done = gold['done']
    assert done.shape == (17, 5) and gold['snap_steps'].tolist() == [3, 6, 11, 17]
    assert (done.sum(1) >= 2).any() and (~done.any(0)).any()
    assert (done[1:] & done[:-1]).any()  # an episode of length 1


@pytest.mark.parametrize('S', [3, 6, 11, 17])
def test_snapshot_and_sample_reproduce_the_reference(gold, S):
    ring = _replay(gold, S)
    snap = ring.snapshot()
    assert sorted(snap) == sorted(k[len(f's{S}_snap_'):] for k in gold if k.startswith(f's{S}_snap_'))
    for k, v in snap.items():
        _same(v, gold[f's{S}_snap_{k}'], k)
    for cname, cfg in onp.GOLDEN_CONFIGS.items():
        pre = f's{S}_{cname}_'
        draws = {k[len(pre) + 5:]: v for k, v in gold.items() if k.startswith(pre + 'draw_')}
        out, idxs, vg, ag = gco.sample(snap, cfg, draws)
        assert list(out) == gold[pre + 'keys'].tolist()
        for k, v in out.items():
            _same(v, gold[pre + 'out_' + k], f'{cname} {k}')
        # and through the ring's own sample (which drops the snapshot's terminals)
        out2 = ring.sample(cfg, draws)[0]
        assert list(out2) == [k for k in out if k != 'terminals']


def test_header_and_source_are_wired_into_the_build():
    mk = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert 'online.hip' in mk and 'ogbx_online.h' in mk
    hdr = open(os.path.join(ROOT, 'include', 'ogbx_online.h')).read()
    assert re.search(r'#define\s+OGBX_ONLINE_API_VERSION\s+1\b', hdr)
    text = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    exports = sorted(set(re.findall(r'\b(ogbx_online_[a-z0-9_]+)\s*\(', text)))
    assert exports == ['ogbx_online_api_version', 'ogbx_online_clear', 'ogbx_online_gc_sample', 'ogbx_online_insert']
    # every export of the header is in the built library and bound by the Python layer
    from ogbench_amd import _lib
    from ogbench_amd import datasets as D

    L = D._bind()
    assert L is _lib.lib()
    for fn in exports:
        assert hasattr(L, fn) and getattr(L, fn).argtypes is not None, fn
    assert L.ogbx_online_api_version() == 1
    assert ogbench_amd_exports()


def ogbench_amd_exports():
    import ogbench_amd

    return 'GCReplayBuffer' in ogbench_amd.__all__ and ogbench_amd.GCReplayBuffer is ogbench_amd.datasets.GCReplayBuffer
