"""CPU: the column rejects of the replay and ring entry points
(ogbx_replay_sample, ogbx_online_gc_sample, ogbx_online_hgc_sample and
ogbx_online_insert), driven through ctypes on libogbx.so.

The pattern of test_gc_args_cpu.py: every case starts from an argument set the
entry point would accept, violates what its id names and expects OGBX_EINVAL
with exactly the message of that condition.  Every check here runs before the
entry point's first HIP call and nothing dereferences the device pointers before
the reject, so they hold host addresses.  Every case is a reject: an accepted
call would launch a kernel on those addresses (the GPU suites cover the
accepting side).

The three sample entry points report a null column pointer on its own and
before a bad descriptor, and a bad descriptor before a low stride, column by
column (the ogbx_gc_* / ogbx_trl_* entry points fold the first two together and
test the stride first: test_gc_args_cpu.py, test_trl_cpu.py).
"""

import ctypes
import types

import pytest

from ogbench_amd import _lib
from ogbench_amd import datasets as D

REPLAY, RING_GC, RING_HGC = 'ogbx_replay_sample', 'ogbx_online_gc_sample', 'ogbx_online_hgc_sample'
SAMPLERS = (REPLAY, RING_GC, RING_HGC)
INSERT = 'ogbx_online_insert'

_HOST = (ctypes.c_double * 64)()  # stands in for every device buffer; never read or written
ADDR = ctypes.addressof(_HOST)

# a select code every entry point takes, and the codes nearest its allowed set that it refuses
BAD_SELECTS = {REPLAY: (2, -1), RING_GC: (1, 4), RING_HGC: (1, 10, -1)}
MAX_COLS = {REPLAY: ('1 to 16 columns', 16), RING_GC: ('0 to 16 columns', 16), RING_HGC: ('0 to 32 columns', 32),
            INSERT: ('0 to 16 columns', 16)}


def good():
    a = types.SimpleNamespace()
    a.ring = D.OnlineRing(4, 8, 3, ADDR, ADDR, ADDR)
    a.cfg = D.GcConfig(0.2, 0.625, 0.99, 0.0, 1.0, 0.99, 1, 0, 0, 0, 1, 0)
    a.hcfg = D.HgcConfig(25, 25, 25, 1, 0, 0.9, ADDR, ADDR, ADDR, ADDR)
    a.out = D.HgcOutputs(None, None, None, None, *[ADDR] * 9)
    a.cols = [D.GcColumn(ADDR, ADDR, 16, 0, 0), D.GcColumn(ADDR, ADDR, 8, 0, 32)]
    a.ins = [D.ReplayInsertColumn(ADDR, ADDR, None, 4, 4, 4, 0, 0), D.ReplayInsertColumn(ADDR, ADDR, ADDR, 2, 0, 1, 0, 0)]
    a.done = a.alt_select = ADDR
    a.total = 8
    return a


def call(who, a):
    L = D._bind_hgc()
    if who == INSERT:
        arr = (D.ReplayInsertColumn * max(1, len(a.ins)))(*a.ins)
        return L.ogbx_online_insert(a.ring, arr, len(a.ins), a.done, a.alt_select, None)
    arr = (D.GcColumn * max(1, len(a.cols)))(*a.cols)
    cols, n = ctypes.cast(arr, ctypes.c_void_p), len(a.cols)
    if who == REPLAY:
        return L.ogbx_replay_sample(ADDR, 0, 64, cols, n, a.total, None, 1, 0, None, None, None)
    if who == RING_GC:
        batch = D.OnlineBatch(cols, n, 0, a.total, None, None, None, ADDR, ADDR)
        return L.ogbx_online_gc_sample(a.ring, a.cfg, batch, None, None, 1, 0, None)
    assert who == RING_HGC
    return L.ogbx_online_hgc_sample(a.ring, a.cfg, a.hcfg, cols, n, a.total, None, a.out, None, 1, 0, None)


def column(i, **fields):
    """Mutation of gather column i (a sample call) or insert column i."""
    def mutate(a, who):
        for k, v in fields.items():
            setattr((a.ins if who == INSERT else a.cols)[i], k, v)
    return mutate


def both(*mutations):
    def mutate(a, who):
        for m in mutations:
            m(a, who)
    return mutate


def one_too_many(a, who):
    n = MAX_COLS[who][1] + 1
    if who == INSERT:
        a.ins = [D.ReplayInsertColumn(ADDR, ADDR, None, 1, 4, 4, 0, 0) for _ in range(n)]
    else:
        a.cols = [D.GcColumn(ADDR, ADDR, 4, 0, 0) for _ in range(n)]


def no_alt_select(a, who):
    a.alt_select = None


NULL, DESC, STRIDE = 'null column pointer', 'bad column descriptor', 'src_stride below row_bytes'
bad_select = lambda who: BAD_SELECTS[who][0]  # noqa: E731

# (id, entry points, mutation, message after "<entry point>: ")
CASES = (
    [('null_src', SAMPLERS + (INSERT,), column(1, src=None), NULL),
     ('null_dst', SAMPLERS + (INSERT,), column(1, dst=None), NULL),
     ('row_bytes_0', SAMPLERS, column(1, row_bytes=0), DESC),
     ('row_bytes_negative', SAMPLERS, column(1, row_bytes=-4), DESC),
     ('stride_below_row', SAMPLERS, column(1, src_stride=4), STRIDE),
     ('one_column_too_many', SAMPLERS + (INSERT,), one_too_many, lambda who: MAX_COLS[who][0]),
     # precedence inside one column: null pointer, then descriptor, then stride
     ('null_and_bad_select', SAMPLERS, lambda a, who: column(1, src=None, select=bad_select(who))(a, who), NULL),
     ('null_and_stride', SAMPLERS, column(1, dst=None, src_stride=4), NULL),
     ('bad_select_and_stride', SAMPLERS, lambda a, who: column(1, select=bad_select(who), src_stride=4)(a, who), DESC),
     # and column by column: an earlier column's fault is reported whatever a later one holds
     ('bad_select_then_null', SAMPLERS,
      lambda a, who: both(column(0, select=bad_select(who)), column(1, src=None))(a, who), DESC),
     ('stride_then_null', SAMPLERS, both(column(0, src_stride=8), column(1, dst=None)), STRIDE),
     # ogbx_online_insert's own column checks, in their order
     ('row_elems_0', (INSERT,), column(0, row_elems=0), 'row_elems must be > 0'),
     ('row_too_long', (INSERT,), column(0, row_elems=(4 << 20) // 8 + 1), 'a row of more than 4 MiB'),
     ('src_dtype_below', (INSERT,), column(0, src_dtype=-1), 'unknown source dtype'),
     ('src_dtype_above', (INSERT,), column(0, src_dtype=6), 'unknown source dtype'),
     ('dst_dtype_bool', (INSERT,), column(0, dst_dtype=0), 'unknown destination dtype'),
     ('dst_dtype_above', (INSERT,), column(0, dst_dtype=6), 'unknown destination dtype'),
     ('op_unknown', (INSERT,), column(0, op=2), 'unknown op'),
     ('op_negative', (INSERT,), column(0, op=-1), 'unknown op'),
     ('alt_without_alt_select', (INSERT,), no_alt_select, 'a column has alt but the call has no alt_select'),
     ('null_and_row_elems_0', (INSERT,), column(0, src=None, row_elems=0), NULL),
     ('row_elems_0_then_null', (INSERT,), both(column(0, row_elems=0), column(1, src=None)), 'row_elems must be > 0')]
    + [(f'select_{s}', (who,), column(1, select=s), DESC) for who in SAMPLERS for s in BAD_SELECTS[who]]
)


@pytest.mark.parametrize('who,mutate,message', [
    pytest.param(who, m, p, id=f'{who}-{i}') for i, whos, m, p in CASES for who in whos])
def test_reject(who, mutate, message):
    a = good()
    mutate(a, who)
    st = call(who, a)
    assert st == _lib.OGBX_EINVAL
    assert _lib.last_error() == f'{who}: {message(who) if callable(message) else message}'
