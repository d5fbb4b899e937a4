"""CPU: the argument rejects that the dataset and ring samplers word alike --
ogbx_visual_gather / ogbx_online_visual_gather, ogbx_trl_sample /
ogbx_online_trl_sample, ogbx_atc_sample / ogbx_online_atc_sample and the config
and output checks of ogbx_online_hgc_sample against ogbx_hgc_sample -- driven
through ctypes on libogbx.so.

The pattern of test_gc_args_cpu.py and test_buffer_args_cpu.py: every case
starts from an argument set the entry point would accept, violates what its id
names and expects OGBX_EINVAL with exactly the message of that condition.
Every check here runs before the entry point's first HIP call and nothing
dereferences the device pointers before the reject, so they hold host
addresses.  Every case is a reject: an accepted call would launch a kernel on
those addresses (the GPU suites cover the accepting side).  The two-fault cases
pin the order in which an entry point runs its checks.
"""

import ctypes
import types

import pytest

from ogbench_amd import _lib, _online_atc, _online_trl, _online_visual
from ogbench_amd import datasets as D

VIS, RING_VIS = 'ogbx_visual_gather', 'ogbx_online_visual_gather'
TRL, RING_TRL = 'ogbx_trl_sample', 'ogbx_online_trl_sample'
HGC, RING_HGC = 'ogbx_hgc_sample', 'ogbx_online_hgc_sample'
ATC, RING_ATC = 'ogbx_atc_sample', 'ogbx_online_atc_sample'
GATHERS, TRLS, ATCS = (VIS, RING_VIS), (TRL, RING_TRL), (ATC, RING_ATC)

_HOST = (ctypes.c_double * 64)()  # stands in for every device buffer; never read or written
ADDR = ctypes.addressof(_HOST)


def good():
    a = types.SimpleNamespace()
    a.buf = D.GcBuffer(30, ADDR, 27, ADDR, ADDR, ADDR, 10, 9, 9)
    a.ring = D.OnlineRing(3, 6, 4, ADDR, ADDR, ADDR)
    # a TRL config: the value goal always from the trajectory, never the sample itself
    a.cfg = D.GcConfig(0.0, 1.0, 0.99, 0.0, 1.0, 0.99, 1, 0, 0, 0, 1, 0)
    a.hcfg = D.HgcConfig(25, 25, 25, 1, 0, 0.9, ADDR, ADDR, ADDR, ADDR)
    a.use_hcfg = True  # the gathers take hcfg or NULL
    a.hout = D.HgcOutputs(None, None, None, None, *[ADDR] * 9)
    a.tout = D.TrlOutputs(*[ADDR] * 9)
    a.cols = [D.GcColumn(ADDR, ADDR, 16, 0, 0), D.GcColumn(ADDR, ADDR, 8, 4, 32)]
    a.vis = [D.VisualColumn(ADDR, ADDR, 8, 8, 3, 0, 1, 1), D.VisualColumn(ADDR, ADDR, 8, 8, 3, 2, 1, 0)]
    a.rvis = [_online_visual.OnlineVisualColumn(ADDR, ADDR, ADDR, 8, 8, 3, 0, 1, 1),
              _online_visual.OnlineVisualColumn(ADDR, None, ADDR, 8, 8, 3, 2, 1, 0)]
    a.indices = D.VisualIndices(ADDR, ADDR, ADDR, ADDR)
    a.total = 2
    a.frame_stack, a.padding = 3, 3
    a.crop_from, a.draw_crop, a.crop_out = None, 1, ADDR
    a.P = ADDR
    a.record = D.GcDrawRecord(*[ADDR] * 11)
    # the ATC pair: an image column that crops, a valid(2) table of 5 rows, every output asked for
    a.atc = D.AtcColumn(ADDR, ADDR, ADDR, 8, 8, 3, 1)
    a.aout = D.AtcOutputs(ADDR, ADDR, ADDR, ADDR)
    a.k, a.valid, a.num_valid, a.W = 2, ADDR, 5, ADDR
    return a


def call(who, a):
    L = D._bind_hgc()
    if who in ATCS:
        rest = (a.frame_stack, a.padding, None, None, a.crop_from, a.draw_crop, 1, 0, a.aout, None)
        if who == ATC:
            return L.ogbx_atc_sample(a.buf, a.atc, a.total, a.k, a.valid, a.num_valid, *rest)
        return _online_atc.bind().ogbx_online_atc_sample(a.ring, a.k, a.W, a.P, a.atc, a.total, *rest)
    if who in GATHERS:
        hcfg = a.hcfg if a.use_hcfg else None
        colv = a.vis if who == VIS else a.rvis
        arr = None
        if colv is not None:
            kind = D.VisualColumn if who == VIS else _online_visual.OnlineVisualColumn
            arr = ctypes.cast((kind * max(1, len(colv)))(*colv), ctypes.c_void_p)
        n = len(colv) if colv is not None else 1
        rest = (arr, n, a.total, a.indices, a.frame_stack, a.padding, a.crop_from, a.draw_crop, 1, 0, a.crop_out, None)
        if who == VIS:
            return L.ogbx_visual_gather(a.buf, hcfg, *rest)
        return _online_visual.bind().ogbx_online_visual_gather(a.ring, hcfg, *rest)
    arr = (D.GcColumn * max(1, len(a.cols)))(*a.cols)
    cols, n = ctypes.cast(arr, ctypes.c_void_p), len(a.cols)
    if who == TRL:
        return L.ogbx_trl_sample(a.buf, a.cfg, cols, n, a.total, 1, None, None, 1, 0, a.tout, a.record, None, None)
    if who == RING_TRL:
        return _online_trl.bind().ogbx_online_trl_sample(a.ring, a.P, a.cfg, cols, n, a.total, None, None, 1, 0,
                                                         a.tout, a.record, None, None)
    a.cols[1].select = 2  # the midpoint selector is TRL's
    arr = (D.GcColumn * len(a.cols))(*a.cols)
    cols = ctypes.cast(arr, ctypes.c_void_p)
    if who == HGC:
        return L.ogbx_hgc_sample(a.buf, a.cfg, a.hcfg, cols, n, a.total, 1, None, 1, 0, a.hout, None, None)
    assert who == RING_HGC
    return L.ogbx_online_hgc_sample(a.ring, a.cfg, a.hcfg, cols, n, a.total, None, a.hout, None, 1, 0, None)


def setter(path, value):
    """Mutation: a.<path> = value (path like 'hcfg.low_discount' or 'total')."""
    def mutate(a, who):
        obj, names = a, path.split('.')
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value)
    return mutate


def column(i, **fields):
    """Mutation of image column i of the gather `who`."""
    def mutate(a, who):
        for k, v in fields.items():
            setattr((a.vis if who == VIS else a.rvis)[i], k, v)
    return mutate


def both(*mutations):
    def mutate(a, who):
        for m in mutations:
            m(a, who)
    return mutate


def columns(n):
    def mutate(a, who):
        a.vis = [D.VisualColumn(ADDR, ADDR, 8, 8, 3, 0, 0, 0) for _ in range(n)]
        a.rvis = [_online_visual.OnlineVisualColumn(ADDR, None, ADDR, 8, 8, 3, 0, 0, 0) for _ in range(n)]
    return mutate


def null_columns(a, who):
    a.vis = a.rvis = None


no_hcfg = setter('use_hcfg', False)
NULLARG, SELECT, MISSING = 'null argument', 'selector out of range', 'a column selects through a missing index output'
SHAPE, STACK = 'bad image shape', 'frame_stack must be in 1..8'
RECORD, SCALAR, TABLES = 'incomplete draw record', 'missing scalar output', 'missing reward/mask tables'
VALUE_GOALS = 'a TRL batch needs value_p_curgoal == 0 and no random value goals (value_traj_thresh >= 1)'

ATC_TOO_LARGE = both(setter('atc.height', 32768), setter('atc.width', 32768), setter('atc.px_bytes', 2))

# (id, entry points, mutation, message after "<entry point>: ")
CASES = (
    # ---- the two image gathers
    [('null_indices', GATHERS, setter('indices', None), NULLARG),
     ('null_buf', (VIS,), setter('buf', None), NULLARG),
     ('null_columns', GATHERS, null_columns, NULLARG),
     ('null_idxs', GATHERS, setter('indices.idxs', None), 'indices->idxs is required'),
     ('17_columns', (VIS,), columns(17), 'at most 16 columns'),
     ('17_columns', (RING_VIS,), columns(17), '1 to 16 columns'),
     ('0_columns', (RING_VIS,), columns(0), '1 to 16 columns'),
     ('total_0', GATHERS, setter('total', 0), 'total must be > 0'),
     ('frame_stack_0', GATHERS, setter('frame_stack', 0), STACK),
     ('frame_stack_9', GATHERS, setter('frame_stack', 9), STACK),
     ('padding_negative', GATHERS, setter('padding', -1), 'padding must be >= 0'),
     ('crop_out_without_offsets', GATHERS, setter('draw_crop', 0), 'crop_out without crop offsets'),
     ('null_src', GATHERS, column(1, src=None), 'null column pointer'),
     ('null_dst', GATHERS, column(1, dst=None), 'null column pointer'),
     ('height_0', GATHERS, column(1, height=0), SHAPE),
     ('width_0', GATHERS, column(1, width=0), SHAPE),
     ('px_bytes_0', GATHERS, column(1, px_bytes=0), SHAPE),
     ('select_negative', GATHERS, column(1, select=-1), SELECT),
     ('select_10', GATHERS, column(1, select=10), SELECT),
     ('select_4_without_hcfg', GATHERS, both(no_hcfg, column(1, select=4)), SELECT),
     ('select_1', (RING_VIS,), column(1, select=1), SELECT),
     ('select_2_without_value_goals', GATHERS, setter('indices.value_goal_idxs', None), MISSING),
     ('select_3_without_actor_goals', GATHERS, both(column(1, select=3), setter('indices.actor_goal_idxs', None)),
      MISSING),
     ('select_6_without_low_goals', GATHERS, both(column(1, select=6), setter('indices.low_value_goal_idxs', None)),
      MISSING),
     ('select_5_without_value_goals', GATHERS, both(column(1, select=5), setter('indices.value_goal_idxs', None)),
      MISSING),
     ('select_9_without_actor_goals', GATHERS, both(column(1, select=9), setter('indices.actor_goal_idxs', None)),
      MISSING),
     ('image_too_large', GATHERS, column(1, height=32768, width=32768, px_bytes=2), 'image too large'),
     ('row_too_wide', GATHERS, column(1, height=1, width=70000, px_bytes=1, stack=0), 'image row too wide to stage'),
     ('too_many_pairs', GATHERS, setter('total', 1 << 31), 'too many (sample, column) pairs for one launch')]
    + [(f'negative_{k}', GATHERS, setter(f'hcfg.{k}', -1), 'negative subgoal steps')
       for k in ('value_subgoal_steps', 'low_subgoal_steps', 'actor_subgoal_steps')]
    # ---- the two TRL samplers
    + [(f'record_without_{k}', TRLS, setter(f'record.{k}', None), RECORD) for k in D._DRAW_ORDER[1:]]
    + [('value_p_curgoal', (RING_TRL,), setter('cfg.value_p_curgoal', 0.1), VALUE_GOALS),
       ('value_traj_thresh', (RING_TRL,), setter('cfg.value_traj_thresh', 0.5), VALUE_GOALS),
       ('value_cur_is_one', (RING_TRL,), setter('cfg.value_cur_is_one', 1), VALUE_GOALS)]
    # ---- HGC over the ring
    + [(f'null_{k}', (RING_HGC,), setter(f'hcfg.{k}', None), TABLES)
       for k in ('hv_mask_table', 'hv_reward_table', 'lv_mask_table', 'lv_reward_table')]
    + [(f'{k}_0', (RING_HGC,), setter(f'hcfg.{k}', 0), 'subgoal steps must be >= 1')
       for k in ('value_subgoal_steps', 'low_subgoal_steps', 'actor_subgoal_steps')]
    + [(f'low_discount_{v}', (RING_HGC,), setter('hcfg.low_discount', v), 'low_discount must be in (0, 1)')
       for v in (0.0, 1.0)]
    + [(f'null_out_{k}', (RING_HGC,), setter(f'hout.{k}', None), SCALAR) for k in D._HGC_SCALARS[4:]]
    # two faults: ogbx_hgc_sample looks at its outputs first, the ring's at its config first
    + [('outputs_against_tables', (HGC,), both(setter('hout.masks', None), setter('hcfg.hv_mask_table', None)), SCALAR),
       ('outputs_against_low_discount', (HGC,), both(setter('hout.rewards', None), setter('hcfg.low_discount', 1.0)),
        SCALAR),
       ('tables_against_outputs', (RING_HGC,), both(setter('hout.masks', None), setter('hcfg.hv_mask_table', None)),
        TABLES),
       ('subgoal_steps_against_outputs', (RING_HGC,),
        both(setter('hout.masks', None), setter('hcfg.low_subgoal_steps', 0)), 'subgoal steps must be >= 1'),
       ('low_discount_against_outputs', (RING_HGC,), both(setter('hout.rewards', None), setter('hcfg.low_discount', 1.0)),
        'low_discount must be in (0, 1)')]
    # ---- the two ATC samplers
    + [(f'atc_null_{k}', ATCS, setter(f'atc.{k}', None), 'null column pointer') for k in ('src', 'anchor', 'positive')]
    + [(f'atc_{k}_0', ATCS, setter(f'atc.{k}', 0), SHAPE) for k in ('height', 'width', 'px_bytes')]
    + [('atc_total_0', ATCS, setter('total', 0), 'total must be > 0'),
       ('atc_k_negative', ATCS, setter('k', -1), 'k must be >= 0'),
       ('atc_frame_stack_0', ATCS, setter('frame_stack', 0), STACK),
       ('atc_frame_stack_9', ATCS, setter('frame_stack', 9), STACK),
       ('atc_padding_negative', ATCS, setter('padding', -1), 'padding must be >= 0'),
       ('atc_crop_from_output_without_offsets', ATCS, setter('draw_crop', 0), 'crop_from output without crop offsets'),
       ('atc_image_too_large', ATCS, ATC_TOO_LARGE, 'image too large'),
       ('atc_row_too_wide', ATCS, both(setter('atc.height', 1), setter('atc.width', 70000), setter('atc.px_bytes', 1),
                                       setter('frame_stack', 1)), 'image row too wide to stage'),
       ('atc_too_many_pairs', ATCS, setter('total', 1 << 31), 'too many (sample, side) pairs for one launch'),
       # two faults: the order of the shared checks, and ogbx_atc_sample's valid(k) checks between its two blocks
       ('atc_total_against_k', ATCS, both(setter('total', 0), setter('k', -1)), 'total must be > 0'),
       ('atc_padding_against_too_large', ATCS, both(setter('padding', -1), ATC_TOO_LARGE), 'padding must be >= 0'),
       ('atc_empty_valid_against_too_large', (ATC,), both(setter('num_valid', 0), ATC_TOO_LARGE), 'valid(k) is empty')]
)


@pytest.mark.parametrize('who,mutate,message', [
    pytest.param(who, m, p, id=f'{who}-{i}') for i, whos, m, p in CASES for who in whos])
def test_reject(who, mutate, message):
    a = good()
    mutate(a, who)
    st = call(who, a)
    assert st == _lib.OGBX_EINVAL
    assert _lib.last_error() == f'{who}: {message}'
