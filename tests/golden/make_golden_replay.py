"""Golden fixtures for the replay buffer, from the reference's own ReplayBuffer
(impls/utils/datasets.py:86-146).

Reuses make_golden_gc's loader of the reference modules (its tree_map /
FrozenDict stand-ins suffice).  Saves arrays only
(tests/golden/replay_golden.npz).  Values are small integers (stored in the
leaf's dtype) unless a scenario is about rounding, so the file stays a few KB.

Scenarios
  ring5     max_size 5, the SAC layout; 7 adds from empty through the wrap:
            ``ring5_in_<key>`` [7, ...], the (pointer, size) trace
            ``ring5_pointer`` / ``ring5_size`` [8] (before the first add and
            after each) and the buffers after each add ``ring5_snap_<key>``
            [7, 5, ...].  Then clear(): ``clear_state`` (pointer, size) and the
            exception sample() raises, ``clear_error``.
  ring300   max_size 300, keys observations / rewards; 650 adds, up to the
            size = max_size - 1 plateau: inputs, trace [651], final buffers
            ``ring300_buf_<key>``.
  dtypes    max_size 5; leaves float64 (2,), float32 (3,), a Python float, a
            uint8 image (4, 4, 3), an int64 scalar; 4 adds whose leaves have
            other dtypes than their columns (``dtypes_add<i>_<key>``, each in
            its own dtype) and the final buffers ``dtypes_buf_<key>``.
  init<n>   create_from_initial_dataset with n = 3, 4, 5 rows into max_size 5:
            ``init<n>_in_<key>``, the state before and after one add
            (``init<n>_pointer`` / ``_size`` [2], or [1] when the add raised),
            the added transition ``init<n>_add_<key>``, the final buffers and,
            for n = 5, ``init5_error`` (IndexError) and a recorded sample over
            the full buffer (``init5_idxs``, ``init5_out_<key>``).
  sample_regular / sample_compact
            max_size 300 after 120 adds, with / without next_observations:
            the buffers, ``<s>_state`` (pointer, size), the recorded
            np.random.randint draw ``<s>_idxs`` of sample(64), the batch
            ``<s>_out_<key>`` and its key order ``<s>_keys``; and get_subset at
            rows including size - 1: ``<s>_sub_idxs``, ``<s>_sub_out_<key>``.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_gc as gg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def ints(rng, shape, dtype, lo=-9, hi=10):
    return rng.randint(lo, hi, shape).astype(dtype)


def sac_example():
    return dict(observations=np.zeros(3, np.float32), actions=np.zeros(2, np.float32), rewards=0.0, masks=1.0,
                next_observations=np.zeros(3, np.float32))


def sac_rows(rng, n):
    return dict(observations=ints(rng, (n, 3), np.float32), actions=ints(rng, (n, 2), np.float32),
                rewards=ints(rng, (n,), np.float64), masks=ints(rng, (n,), np.float64, 0, 2),
                next_observations=ints(rng, (n, 3), np.float32))


def add_rows(rb, rows, n, snaps=None):
    ptr, size = [rb.pointer], [rb.size]
    for i in range(n):
        rb.add_transition({k: v[i] for k, v in rows.items()})
        ptr.append(rb.pointer)
        size.append(rb.size)
        if snaps is not None:
            for k in rb._dict:
                snaps.setdefault(k, []).append(rb._dict[k].copy())
    return np.array(ptr, np.int64), np.array(size, np.int64)


def main():
    _, dsm, _ = gg.reference_modules()
    RB = dsm.ReplayBuffer
    rng = np.random.RandomState(8614)
    out = {}

    # ring5, then clear
    rb = RB.create(sac_example(), 5)
    assert rb['rewards'].dtype == np.float64 and rb['observations'].dtype == np.float32
    rows = sac_rows(rng, 7)
    snaps = {}
    out['ring5_pointer'], out['ring5_size'] = add_rows(rb, rows, 7, snaps)
    assert (rb.pointer, rb.size) == (2, 4)  # the size quirk: max(pointer, size) after the modulo
    for k, v in rows.items():
        out[f'ring5_in_{k}'] = v
        out[f'ring5_snap_{k}'] = np.stack(snaps[k])
    rb.clear()
    out['clear_state'] = np.array([rb.pointer, rb.size], np.int64)
    try:
        rb.sample(4)
    except ValueError:
        out['clear_error'] = np.array('ValueError')
    else:
        raise AssertionError('the reference sampled an empty buffer')

    # ring300
    rb = RB.create(dict(observations=np.zeros(2, np.float32), rewards=0.0), 300)
    rows = dict(observations=ints(rng, (650, 2), np.float32), rewards=ints(rng, (650,), np.float64))
    out['ring300_pointer'], out['ring300_size'] = add_rows(rb, rows, 650)
    assert (rb.pointer, rb.size) == (50, 299)
    for k, v in rows.items():
        out[f'ring300_in_{k}'] = v
        out[f'ring300_buf_{k}'] = rb._dict[k].copy()

    # dtypes
    example = dict(a64=np.zeros(2, np.float64), b32=np.zeros(3, np.float32), pyfloat=0.0,
                   image=np.zeros((4, 4, 3), np.uint8), count=np.int64(0))
    rb = RB.create(example, 5)
    assert [rb[k].dtype for k in example] == [np.float64, np.float32, np.float64, np.uint8, np.int64]
    adds = [
        dict(a64=np.array([1.5, -2.25], np.float32), b32=np.array([0.1, 1.0 / 3.0, -2.0 / 3.0], np.float64),
             pyfloat=np.float32(0.1), image=ints(rng, (4, 4, 3), np.int64, 0, 256), count=np.float64(2.9)),
        dict(a64=np.array([7, -3], np.int64), b32=np.array([16777217, -5, 9], np.int64),
             pyfloat=np.int32(-4), image=rng.uniform(0, 255.9, (4, 4, 3)).astype(np.float32),
             count=np.float32(-2.9)),
        dict(a64=np.array([200, 3], np.uint8), b32=np.array([1, 0, 1], np.bool_),
             pyfloat=np.bool_(True), image=rng.uniform(0, 255.9, (4, 4, 3)).astype(np.float64),
             count=np.uint8(250)),
        dict(a64=np.array([2 ** 53 + 1, -1], np.int64), b32=np.array([1e-3, 2.5, 1e10], np.float64),
             pyfloat=np.int64(2 ** 40 + 1), image=ints(rng, (4, 4, 3), np.int32, 0, 256), count=np.bool_(True)),
    ]
    for i, tr in enumerate(adds):
        rb.add_transition(tr)
        for k, v in tr.items():
            out[f'dtypes_add{i}_{k}'] = np.asarray(v)
    assert (rb.pointer, rb.size) == (4, 4)
    for k in example:
        out[f'dtypes_buf_{k}'] = rb._dict[k].copy()

    # create_from_initial_dataset: shorter than, one less than, equal to max_size
    for n in (3, 4, 5):
        init = sac_rows(rng, n)
        rb = RB.create_from_initial_dataset(init, 5)
        for k, v in init.items():
            out[f'init{n}_in_{k}'] = v
        ptr, size = [rb.pointer], [rb.size]
        one = sac_rows(rng, 1)
        for k, v in one.items():
            out[f'init{n}_add_{k}'] = v
        try:
            rb.add_transition({k: v[0] for k, v in one.items()})
            ptr.append(rb.pointer)
            size.append(rb.size)
            assert n < 5
        except IndexError:
            assert n == 5
            out['init5_error'] = np.array('IndexError')
            np.random.seed(305)
            with gg.Recorder() as rec:
                batch = rb.sample(16)
            assert [name for name, _ in rec.log] == ['randint']
            out['init5_idxs'] = rec.log[0][1].astype(np.int64)
            assert out['init5_idxs'].max() == 4  # the full buffer is covered
            for k, v in batch.items():
                out[f'init5_out_{k}'] = np.asarray(v)
        out[f'init{n}_pointer'] = np.array(ptr, np.int64)
        out[f'init{n}_size'] = np.array(size, np.int64)
        for k in init:
            out[f'init{n}_buf_{k}'] = rb._dict[k].copy()

    # sampling: regular and compact buffers, size < max_size
    for name, example in (('sample_regular', sac_example()),
                          ('sample_compact', dict(observations=np.zeros(3, np.float32),
                                                  actions=np.zeros(2, np.float32)))):
        rb = RB.create(example, 300)
        rows = {k: v for k, v in sac_rows(rng, 120).items() if k in example}
        add_rows(rb, rows, 120)
        assert (rb.pointer, rb.size) == (120, 120)
        for k in example:
            out[f'{name}_buf_{k}'] = rb._dict[k].copy()
        out[f'{name}_state'] = np.array([rb.pointer, rb.size], np.int64)
        np.random.seed(306)
        with gg.Recorder() as rec:
            batch = rb.sample(64)
        assert [n_ for n_, _ in rec.log] == ['randint']
        out[f'{name}_idxs'] = rec.log[0][1].astype(np.int64)
        out[f'{name}_keys'] = np.array(list(batch.keys()))
        for k, v in batch.items():
            out[f'{name}_out_{k}'] = np.asarray(v)
        sub = np.array([119, 0, 118, 119, 57], np.int64)  # size - 1 while size < max_size
        out[f'{name}_sub_idxs'] = sub
        for k, v in rb.get_subset(sub).items():
            out[f'{name}_sub_out_{k}'] = np.asarray(v)
    # the compact clamp is the current size - 1, not max_size - 1
    assert np.array_equal(out['sample_compact_sub_out_next_observations'][0], out['sample_compact_buf_observations'][119])

    path = os.path.join(OUT, 'replay_golden.npz')
    np.savez_compressed(path, **out)
    print('replay golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
