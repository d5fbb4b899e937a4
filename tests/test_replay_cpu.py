"""CPU tests of the replay-buffer restatement (tests/replay_np.py) against the
reference's recorded behaviour (tests/golden/replay_golden.npz, built by
tests/golden/make_golden_replay.py), and of the closed-form header rule."""

import os
import re

import numpy as np
import pytest

import replay_np as rnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'replay_golden.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _same(got, exp, what=''):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    np.testing.assert_array_equal(got, exp, err_msg=what)


def test_closed_form_equals_sequential_for_every_state_of_a_buffer_of_7():
    n = 7
    for pointer in range(n):
        for size in range(n):
            for m in range(n + 1):
                assert rnp.closed_state(pointer, size, m, n) == rnp.sequential_state(pointer, size, m, n), \
                    (pointer, size, m)


def test_the_size_quirk(gold):
    # a buffer of 5 after 7 adds: pointer 2, size 4 -- the last row is never drawn
    assert (gold['ring5_pointer'][-1], gold['ring5_size'][-1]) == (2, 4)
    assert gold['ring300_size'].max() == 299 and gold['ring300_pointer'][-1] == 50


@pytest.mark.parametrize('chunk', [1, 2, 3, 5])
def test_ring5_in_batches(gold, chunk):
    rows = rnp.scenario(gold, 'ring5', 'in')
    snaps = rnp.scenario(gold, 'ring5', 'snap')
    rb = rnp.ReplayNp.create({k: v[0] for k, v in rows.items()}, 5)
    assert [rb.cols[k].dtype for k in rows] == [v.dtype for v in snaps.values()]
    done = 0
    while done < 7:
        m = min(chunk, 7 - done)
        rb.add_transitions({k: v[done:done + m] for k, v in rows.items()})
        done += m
        assert (rb.pointer, rb.size) == (gold['ring5_pointer'][done], gold['ring5_size'][done])
        for k in rows:
            _same(rb.cols[k], snaps[k][done - 1], k)


@pytest.mark.parametrize('chunk', [1, 63, 65, 257, 300])
def test_ring300_in_batches(gold, chunk):
    rows = rnp.scenario(gold, 'ring300', 'in')
    rb = rnp.ReplayNp.create({k: v[0] for k, v in rows.items()}, 300)
    done = 0
    while done < 650:
        m = min(chunk, 650 - done)
        rb.add_transitions({k: v[done:done + m] for k, v in rows.items()})
        done += m
        assert (rb.pointer, rb.size) == (gold['ring300_pointer'][done], gold['ring300_size'][done])
    for k, v in rnp.scenario(gold, 'ring300', 'buf').items():
        _same(rb.cols[k], v, k)


def test_keep_mask_equals_adding_the_kept_rows(gold):
    rows = rnp.scenario(gold, 'ring300', 'in')
    keep = np.random.RandomState(3).rand(650) < 0.4
    a = rnp.ReplayNp.create({k: v[0] for k, v in rows.items()}, 300)
    b = rnp.ReplayNp.create({k: v[0] for k, v in rows.items()}, 300)
    for lo in range(0, 650, 130):
        sl = slice(lo, lo + 130)
        a.add_transitions({k: v[sl] for k, v in rows.items()}, keep[sl])
        for i in np.flatnonzero(keep[sl]) + lo:
            b.add_transitions({k: v[i:i + 1] for k, v in rows.items()})
        assert (a.pointer, a.size) == (b.pointer, b.size)
    for k in rows:
        _same(a.cols[k], b.cols[k], k)


def test_casts_across_dtypes(gold):
    buf = rnp.scenario(gold, 'dtypes', 'buf')
    rb = rnp.ReplayNp({k: np.zeros_like(v) for k, v in buf.items()})
    for i in range(4):
        tr = rnp.scenario(gold, 'dtypes', f'add{i}')
        assert any(tr[k].dtype != buf[k].dtype for k in buf)
        rb.add_transitions({k: v[None] for k, v in tr.items()})
    assert (rb.pointer, rb.size) == (4, 4)
    for k, v in buf.items():
        _same(rb.cols[k], v, k)
    assert buf['count'].tolist()[:4] == [2, -2, 250, 1]  # float -> int truncates toward zero
    assert buf['b32'][1, 0] == np.float32(16777216)  # int64 -> float32 rounds to nearest even


@pytest.mark.parametrize('n', [3, 4, 5])
def test_create_from_initial_dataset(gold, n):
    init = rnp.scenario(gold, f'init{n}', 'in')
    rb = rnp.ReplayNp.create_from_initial_dataset(init, 5)
    assert (rb.pointer, rb.size) == (gold[f'init{n}_pointer'][0], gold[f'init{n}_size'][0]) == (n, n)
    one = rnp.scenario(gold, f'init{n}', 'add')
    if n == 5:
        assert str(gold['init5_error']) == 'IndexError'
        with pytest.raises(IndexError):
            rb.add_transitions(one)
        got = rb.get_subset(gold['init5_idxs'])
        for k, v in rnp.scenario(gold, 'init5', 'out').items():
            _same(got[k], v, k)
    else:
        rb.add_transitions(one)
        assert (rb.pointer, rb.size) == (gold[f'init{n}_pointer'][1], gold[f'init{n}_size'][1])
    for k, v in rnp.scenario(gold, f'init{n}', 'buf').items():
        _same(rb.cols[k], v, k)


def test_clear(gold):
    assert gold['clear_state'].tolist() == [0, 0] and str(gold['clear_error']) == 'ValueError'


@pytest.mark.parametrize('name', ['sample_regular', 'sample_compact'])
def test_sample_and_subset(gold, name):
    pointer, size = gold[f'{name}_state'].tolist()
    rb = rnp.ReplayNp(rnp.scenario(gold, name, 'buf'), pointer, size)
    assert size < rb.max_size and gold[f'{name}_idxs'].max() < size
    for part, idxs in (('out', gold[f'{name}_idxs']), ('sub_out', gold[f'{name}_sub_idxs'])):
        exp = rnp.scenario(gold, name, part)
        got = rb.get_subset(idxs)
        assert list(got) == list(exp) == gold[f'{name}_keys'].tolist()
        for k, v in exp.items():
            _same(got[k], v, f'{part} {k}')
    assert (gold[f'{name}_sub_idxs'] == size - 1).any()


def test_add_step_composition():
    rng = np.random.RandomState(5)
    n = 9
    rb = rnp.ReplayNp.create(dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), rewards=0.0, masks=1.0,
                                  next_observations=np.zeros(2)), 16)
    obs, nxt, fin = rng.normal(size=(3, n, 2))
    term = rng.rand(n) < 0.3
    done = term | (rng.rand(n) < 0.3)
    rb.add_step(obs, rng.normal(size=(n, 2)).astype(np.float32), rng.normal(size=n), term, nxt, fin, done)
    np.testing.assert_array_equal(rb.cols['masks'][:n], np.where(term, 0.0, 1.0))
    np.testing.assert_array_equal(rb.cols['next_observations'][:n], np.where(done[:, None], fin, nxt))
    assert (rb.pointer, rb.size) == (n, n)


def test_header_and_source_are_wired_into_the_build():
    mk = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert 'replay.hip' in mk and 'ogbx_replay.h' in mk
    hdr = open(os.path.join(ROOT, 'include', 'ogbx_replay.h')).read()
    assert re.search(r'#define\s+OGBX_REPLAY_API_VERSION\s+1\b', hdr)
    for fn in ('ogbx_replay_api_version', 'ogbx_replay_insert', 'ogbx_replay_clear', 'ogbx_replay_sample'):
        assert re.search(rf'\b{fn}\s*\(', hdr), fn
