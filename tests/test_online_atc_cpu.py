"""CPU tests of the restatement of ATC batches over the episode ring
(tests/online_atc_np.py): its closed-form anchor select against the compaction
of the snapshot's terminals (tests/atc_np.valid_idxs) on every step of random
histories and for every k, and its batch against the reference's recorded
behaviour (tests/golden/online_atc_golden.npz, built by
tests/golden/make_golden_online_atc.py)."""

import os
import re

import numpy as np
import pytest

import atc_np as anp
import online_atc_np as oan
import online_np as onp
import online_visual_np as ovn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_atc_golden.npz')
EX1 = dict(observations=np.zeros(2))
FORMS = {'vis': (dict(frame_stack=3, p_aug=1.0), np.zeros(ovn.FRAME, np.uint8)),
         'state': (dict(frame_stack=None, p_aug=None), np.zeros(2))}
SIZES = {(3, 1): 9, (3, 2): 4, (3, 3): 0, (6, 1): 21, (6, 2): 14, (6, 3): 9, (11, 1): 21, (11, 2): 14, (11, 3): 9,
         (17, 1): 22, (17, 2): 15, (17, 3): 10}  # valid(k) at each snapshot of the fixture


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _check_every_step_and_k(N, T, steps, done_of, start=0):
    ring = onp.OnlineNp(EX1, N, T)
    ring.cur_seq[:] = np.array([start] * N, np.uint32).astype(np.int32)
    rng = np.random.RandomState(N * 131 + T)
    sizes = set()
    for step in range(steps):
        with np.errstate(over='ignore'):
            ring.add(dict(observations=rng.normal(size=(N, 2))), done_of(step))
        snap = ring.snapshot()
        for k in range(ring.L):
            exp = anp.valid_idxs(snap, k)
            W, P = oan.table(ring, k)
            assert W.dtype == np.int32 and W.shape == (T, N)
            assert P.dtype == np.int64 and P.shape == (N + 1,) and P[0] == 0 and (np.diff(P) >= 0).all()
            assert P[-1] == len(exp), (step, k, P[-1], len(exp))
            np.testing.assert_array_equal(oan.select(ring, W, P, np.arange(P[-1])), exp, err_msg=f'step {step} k {k}')
            sizes.add((k, int(P[-1])))
        assert oan.table(ring, ring.L)[1][-1] == 0  # no segment holds L + 1 rows
    return sizes


@pytest.mark.parametrize('p', [0.05, 0.5, 1.0])
@pytest.mark.parametrize('N,T', [(1, 1), (1, 2), (3, 4), (5, 7), (7, 9), (2, 5), (6, 8)])
def test_select_equals_brute_compaction(N, T, p):
    """40 steps, every k in 0..L-1, ordinals started at 0xFFFFFFFE so that
    they wrap; p = 1 leaves only episodes of length 1 (anchors at k = 0 only)."""
    rng = np.random.RandomState(1000 * N + 10 * T + int(100 * p))
    sizes = _check_every_step_and_k(N, T, 40, lambda step: rng.rand(N) < p, start=0xFFFFFFFE)
    assert (0, N * T) in sizes  # k = 0: every live row
    if p == 1.0:
        assert all(n == 0 for k, n in sizes if k > 0)


def test_select_from_ordinal_zero_and_across_2_31():
    """Ordinals from 0, and ordinals that cross 2^31 (int32 wraps to negative)
    on a horizon that divides 2^32."""
    for start, T in ((0, 5), (2 ** 31 - 2, 4)):
        rng = np.random.RandomState(3)
        _check_every_step_and_k(3, T, 17, lambda step: rng.rand(3) < 0.4, start=start)


def _replay(gold, form, upto):
    ring = onp.OnlineNp(dict(observations=FORMS[form][1]), ovn.N, ovn.T)
    for t in range(upto):
        ring.add(dict(observations=gold[f'{form}_in_observations'][t]), gold['done'][t])
    return ring


@pytest.mark.parametrize('S', ovn.SNAPS)
def test_restatement_reproduces_the_reference(gold, S):
    assert gold['snap_steps'].tolist() == list(ovn.SNAPS) and gold['ks'].tolist() == [1, 2, 3]
    for k in (1, 2, 3):
        valid = gold[f's{S}_k{k}_valid']
        assert len(valid) == SIZES[S, k]
        for form, (cfg, _) in FORMS.items():
            ring = _replay(gold, form, S)
            W, P = oan.table(ring, k)
            assert P[-1] == len(valid)
            np.testing.assert_array_equal(oan.pick_rows(ring, k), valid)
            np.testing.assert_array_equal(anp.valid_idxs(oan.dataset(ring), k), valid)
            tag = f's{S}_k{k}_{form}'
            if len(valid) == 0:
                assert str(gold[f's{S}_k{k}_error']) == f'No valid ATC indices found for k={k}.'
                with pytest.raises(ValueError, match=f'No valid ATC indices found for k={k}'):
                    oan.batch(ring, cfg, k, dict(pick=np.zeros(1, np.int64)))
                continue
            pick = gold[f'{tag}_draw_pick']
            cf = gold.get(f'{tag}_draw_crop_from')
            assert (cf is not None) == (form == 'vis')
            out, idxs = oan.batch(ring, cfg, k, dict(pick=pick), cf)
            np.testing.assert_array_equal(idxs, gold[f'{tag}_idxs'])
            np.testing.assert_array_equal(oan.select(ring, W, P, pick), idxs)
            assert list(out) == [str(x) for x in gold[f'{tag}_keys']] == list(anp.KEYS)
            for key, v in out.items():
                exp = gold[f'{tag}_out_{key}']
                assert v.dtype == exp.dtype and v.shape == exp.shape, key
                np.testing.assert_array_equal(v, exp, err_msg=f'{tag} {key}')
    assert (S, 3) != (3, 3) or 's3_k3_error' in gold


def test_the_fixture_holds_its_designed_cases(gold):
    """An env without an anchor beside envs that have some; a segment without
    one between two that have some."""
    for S, k in ((3, 2), (6, 3), (11, 3)):
        P = oan.table(_replay(gold, 'state', S), k)[1]
        assert (np.diff(P) == 0).any() and P[-1] > 0, (S, k)
    for S, k in ((6, 1), (11, 1)):
        ring = _replay(gold, 'state', S)
        gaps = 0
        for e in range(ring.N):
            w = [max(E - b + 1 - k, 0) for b, E in oan.segments(ring, e)[2]]
            gaps += any(w[i] == 0 and any(w[:i]) and any(w[i + 1:]) for i in range(len(w)))
        assert gaps >= 1, (S, k)


def test_header_and_source_are_wired_into_the_build():
    mk = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert 'online_atc.hip' in mk and mk.count('ogbx_online_atc.h') == 2  # the header comment and HDRS
    hdr = open(os.path.join(ROOT, 'include', 'ogbx_online_atc.h')).read()
    assert re.search(r'#define\s+OGBX_ONLINE_ATC_API_VERSION\s+1\b', hdr)
    text = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    exports = sorted(set(re.findall(r'\b(ogbx_online_atc_[a-z0-9_]+)\s*\(', text)))
    assert exports == ['ogbx_online_atc_api_version', 'ogbx_online_atc_sample', 'ogbx_online_atc_table',
                       'ogbx_online_atc_table_bytes']
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'ogbx_online_atc.h' in doc and all(f'`{fn}`' in doc for fn in exports)
    from ogbench_amd import _lib, _online_atc

    L = _online_atc.bind()
    assert L is _lib.lib()
    for fn in exports:  # libogbx.so exports the four symbols
        assert hasattr(L, fn) and getattr(L, fn).argtypes is not None, fn
    assert L.ogbx_online_atc_api_version() == _online_atc.ONLINE_ATC_API_VERSION == 1
    tile = int(re.search(r'#define\s+OGBX_ONLINE_ATC_TABLE_TILE\s+(\d+)', hdr).group(1))
    assert tile == _online_atc.ONLINE_ATC_TABLE_TILE == 2048
