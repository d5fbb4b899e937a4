"""CPU: the argument rejects of the GC / HGC sampler entry points (ogbx_gc_* /
ogbx_hgc_*), driven through ctypes on libogbx.so.

Every case starts from an argument set the entry point would accept, violates
exactly one condition and expects OGBX_EINVAL with the message of that
condition -- prefixed with the entry point's name where the check is the entry
point's own.  Every check runs before the entry point's first HIP call and
nothing dereferences the device pointers before the reject, so they hold host
addresses here.  Every case is a reject: an accepted call would launch a
kernel on those addresses (the GPU suite covers the accepting side).
"""

import ctypes
import types

import pytest

from ogbench_amd import _lib
from ogbench_amd import datasets as D

GC, GC_AHEAD, HGC, HGC_AHEAD = 'ogbx_gc_sample', 'ogbx_gc_sample_ahead', 'ogbx_hgc_sample', 'ogbx_hgc_sample_ahead'
ONE_SHOT = (GC, GC_AHEAD, HGC, HGC_AHEAD)
AHEAD = (GC_AHEAD, HGC_AHEAD)
HIER = (HGC, HGC_AHEAD)
PLAN_CREATE = 'ogbx_gc_plan_create'
HGC_SEL = 10  # kHgcSel: select codes 0..9 (include/ogbx.h, ogbx_hgc_sample)

_HOST = (ctypes.c_double * 64)()  # stands in for every device buffer; never read or written
ADDR = ctypes.addressof(_HOST)


def good():
    """Arguments every entry point accepts: 3 trajectories of 10 rows, the last
    row of each invalid, described both by tables and by the closed form."""
    a = types.SimpleNamespace()
    a.buf = D.GcBuffer(30, ADDR, 27, ADDR, ADDR, ADDR, 10, 9, 9)
    a.cfg = D.GcConfig(0.2, 0.625, 0.99, 0.0, 1.0, 0.99, 1, 0, 0, 0, 1, 0)
    a.hcfg = D.HgcConfig(25, 25, 25, 1, 0, 0.9, ADDR, ADDR, ADDR, ADDR)
    a.cols = [D.GcColumn(ADDR, ADDR, 16, 0, 0), D.GcColumn(ADDR, ADDR, 8, 1, 32)]
    a.batch, a.nb = 8, 2
    a.ain, a.aout = ADDR, ADDR + 256
    a.masks = a.rewards = ADDR
    a.out = D.HgcOutputs(None, None, None, None, *[ADDR] * 9)
    a.plan = ctypes.c_void_p()
    return a


def call(who, a):
    L = D._bind_hgc()
    arr = (D.GcColumn * max(1, len(a.cols)))(*a.cols)
    cols, n = ctypes.cast(arr, ctypes.c_void_p), len(a.cols)
    if who == GC:
        return L.ogbx_gc_sample(a.buf, a.cfg, cols, n, a.batch, a.nb, None, 1, 0, None, None, None, a.masks,
                                a.rewards, None, None)
    if who == GC_AHEAD:
        return L.ogbx_gc_sample_ahead(a.buf, a.cfg, cols, n, a.batch, a.nb, 1, 0, a.ain, a.aout, None, None, None,
                                      a.masks, a.rewards, None)
    if who == HGC:
        return L.ogbx_hgc_sample(a.buf, a.cfg, a.hcfg, cols, n, a.batch, a.nb, None, 1, 0, a.out, None, None)
    if who == HGC_AHEAD:
        return L.ogbx_hgc_sample_ahead(a.buf, a.cfg, a.hcfg, cols, n, a.batch, a.nb, 1, 0, a.ain, a.aout, a.out, None)
    assert who == PLAN_CREATE
    hcfg = ctypes.cast(ctypes.pointer(a.hcfg), ctypes.c_void_p) if a.hcfg is not None else None
    return L.ogbx_gc_plan_create(a.buf, a.cfg, hcfg, 1, 1, ctypes.byref(a.plan) if a.plan is not None else None)


def setter(path, value):
    """Mutation: a.<path> = value (path like 'buf.num_rows' or 'batch')."""
    def mutate(a, who):
        obj, names = a, path.split('.')
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value)
    return mutate


def column(field, value):
    """Mutation of the last column; value may depend on the entry point."""
    def mutate(a, who):
        setattr(a.cols[-1], field, value(who) if callable(value) else value)
    return mutate


def same_ahead(a, who):
    a.aout = a.ain


def many_columns(a, who):
    a.cols = [D.GcColumn(ADDR, ADDR, 4, 0, 0) for _ in range(33)]


def gc_only_plan(a, who):
    a.hcfg = None


# (id, entry points, mutation, phrase of ogbx_last_error(); {who} = the entry point's name)
BUFFER_CASES = [
    ('num_rows_0', setter('buf.num_rows', 0), 'empty trajectory buffer'),
    ('null_traj_end', setter('buf.traj_end', None), 'empty trajectory buffer'),
    ('num_valid_0', setter('buf.num_valid', 0), 'no valid transitions'),
    ('period_negative', setter('buf.period', -10), 'inconsistent period fields'),
    ('period_picks_0', setter('buf.period_picks', 0), 'inconsistent period fields'),
    ('period_picks_above_period', setter('buf.period_picks', 11), 'inconsistent period fields'),
    ('period_end_outside', setter('buf.period_end', 10), 'inconsistent period fields'),
    ('period_end_negative', setter('buf.period_end', -1), 'inconsistent period fields'),
    ('period_not_dividing_rows', setter('buf.num_rows', 35), 'inconsistent period fields'),
    ('period_picks_not_num_valid', setter('buf.period_picks', 8), 'inconsistent period fields'),
]
HCFG_CASES = (
    [(f'null_{k}', setter(f'hcfg.{k}', None), '{who}: missing reward/mask tables')
     for k in ('hv_mask_table', 'hv_reward_table', 'lv_mask_table', 'lv_reward_table')]
    + [(f'negative_{k}', setter(f'hcfg.{k}', -1), '{who}: negative subgoal steps')
       for k in ('value_subgoal_steps', 'low_subgoal_steps', 'actor_subgoal_steps')]
    + [(f'low_discount_{v}', setter('hcfg.low_discount', v), '{who}: low_discount must be in (0, 1)')
       for v in (0.0, 1.0, 1.5)]
)
CASES = (
    [('null_buf', ONE_SHOT + (PLAN_CREATE,), setter('buf', None), '{who}: null argument'),
     ('null_cfg', ONE_SHOT + (PLAN_CREATE,), setter('cfg', None), '{who}: null argument'),
     ('null_masks', (GC, GC_AHEAD), setter('masks', None), '{who}: null argument'),
     ('null_rewards', (GC, GC_AHEAD), setter('rewards', None), '{who}: null argument'),
     ('null_hcfg', HIER, setter('hcfg', None), '{who}: null argument'),
     ('null_out', HIER, setter('out', None), '{who}: null argument'),
     ('null_plan_out', (PLAN_CREATE,), setter('plan', None), '{who}: null argument'),
     ('33_columns', ONE_SHOT, many_columns, '{who}: at most 32 columns'),
     ('batch_0', ONE_SHOT, setter('batch', 0), 'batch and num_batches must be > 0'),
     ('num_batches_0', ONE_SHOT, setter('nb', 0), 'batch and num_batches must be > 0'),
     ('col_null_src', ONE_SHOT, column('src', None), '{who}: bad column descriptor'),
     ('col_null_dst', ONE_SHOT, column('dst', None), '{who}: bad column descriptor'),
     ('col_row_bytes_0', ONE_SHOT, column('row_bytes', 0), '{who}: bad column descriptor'),
     ('col_select_negative', ONE_SHOT, column('select', -1), '{who}: bad column descriptor'),
     ('col_select_past_bound', ONE_SHOT, column('select', lambda who: HGC_SEL if who in HIER else 4),
      '{who}: bad column descriptor'),
     ('col_stride_below_row', ONE_SHOT, column('src_stride', 4), '{who}: src_stride below row_bytes'),
     ('1025_samples', AHEAD, setter('batch', 1025), '{who}: at most 1024 samples per call'),
     ('ahead_in_is_ahead_out', AHEAD, same_ahead, '{who}: ahead_in and ahead_out must differ')]
    + [(i, ONE_SHOT + (PLAN_CREATE,), m, p) for i, m, p in BUFFER_CASES]
    + [(i, HIER + (PLAN_CREATE,), m, p) for i, m, p in HCFG_CASES]
    + [(f'null_out_{k}', HIER, setter(f'out.{k}', None), '{who}: missing scalar output')
       for k in D._HGC_SCALARS[4:]]
    # a GCDataset plan (hcfg NULL) checks its buffer all the same
    + [('gc_plan_' + i, (PLAN_CREATE,), lambda a, who, m=m: (gc_only_plan(a, who), m(a, who)), p)
       for i, m, p in BUFFER_CASES[:3]]
)


@pytest.mark.parametrize('who,mutate,phrase', [
    pytest.param(who, m, p, id=f'{who}-{i}') for i, whos, m, p in CASES for who in whos])
def test_reject(who, mutate, phrase):
    a = good()
    mutate(a, who)
    st = call(who, a)
    assert st == _lib.OGBX_EINVAL
    assert phrase.format(who=who) in _lib.last_error()
    assert a.plan is None or a.plan.value is None  # no plan was created


def test_null_plan():
    L = D._bind()
    arr = (D.GcColumn * 1)(D.GcColumn(ADDR, ADDR, 4, 0, 0))
    st = L.ogbx_gc_plan_set_batch(None, 0, ctypes.cast(arr, ctypes.c_void_p), 1, 8, 1, None, None, None, ADDR, ADDR,
                                  None)
    assert st == _lib.OGBX_EINVAL and 'null plan' in _lib.last_error()
    st = L.ogbx_gc_plan_sample(None, 0, 0, None)
    assert st == _lib.OGBX_EINVAL and 'null plan' in _lib.last_error()
    assert L.ogbx_gc_plan_hits(None) == -1
    assert L.ogbx_gc_plan_destroy(None) == _lib.OGBX_OK
