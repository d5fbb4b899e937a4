"""HBM-resident offline datasets and the goal-conditioned sampler.

Batched, device-side counterparts of impls/utils/datasets.py (hliuson/ogbench):

  Dataset    ~ Dataset (datasets.py:36-83): a dict of device tensors with
               ``size``, ``valid_idxs``, ``get_random_idxs``, ``sample``,
               ``get_subset``;
  GCDataset  ~ GCDataset (datasets.py:149-366): ``sample(batch_size, idxs=None,
               evaluation=False)`` returns the same keys as the reference
               (every dataset key, ``next_observations``, ``value_goals``,
               ``actor_goals``, ``masks``, ``rewards``);
  HGCDataset ~ HGCDataset (datasets.py:467-643);
  ATCDataset ~ ATCDataset (datasets.py:369-464): ``sample(batch_size, k,
               evaluation=False)`` returns ``observations`` and
               ``positive_observations``, k rows apart in one trajectory, in
               one launch of ``atc_sample_kernel`` (include/ogbx_atc.h);
  ReplayBuffer ~ ReplayBuffer (datasets.py:86-146): ``create``,
               ``create_from_initial_dataset``, ``add_transition``, ``clear``
               and ``sample`` over the rows held so far; ``add_transitions`` /
               ``add_step`` insert one row per env in one launch of
               ``replay_insert_kernel`` (include/ogbx_replay.h).
  GCReplayBuffer  GCDataset.sample over a growing buffer: a time-major
               episode ring filled one row per env and step
               (``online_insert_kernel``) and sampled as the reference samples
               the snapshot of its live rows (``online_gc_sample_kernel``,
               include/ogbx_online.h); with ``frame_stack`` / ``p_aug`` one
               further launch composes the stacked, cropped image keys from
               the unstacked ring (``online_visual_gather_kernel``,
               include/ogbx_online_visual.h), for ``HGCReplayBuffer`` too;
               with a TRL ``agent_name`` the reference's TRL batch over the
               snapshot (``online_trl_sample_kernel``,
               include/ogbx_online_trl.h); ``sample_atc(batch_size, k)`` is
               ATCDataset.sample over the snapshot
               (``online_atc_sample_kernel``, include/ogbx_online_atc.h).

Every sample is ONE launch of ``gc_sample_kernel`` (libogbx): index draw,
trajectory-end lookup, hindsight goal relabel and the row gathers of every
column are fused.  Random numbers come from a counter-based Philox stream
(key = seed, counter = (sample, call)); the reference's NumPy draws can be
injected bit-exactly through ``draws=`` for parity tests.

Visual datasets (``frame_stack`` / ``p_aug``, as every ``visual-*`` line of
the reference's hyperparameters.sh sets them): the image columns of a batch
-- frame stacks and the random crop -- are written by one further launch,
``visual_gather_kernel`` (``ogbx_visual_gather``, include/ogbx_visual.h), from
the index outputs of the fused launch.  The frames stay unstacked in HBM.
"""

from __future__ import annotations

import ctypes
import operator
import weakref

import numpy as np

from . import _lib, _online_atc, _online_trl, _online_visual
from ._online_visual import OnlineVisualColumn


def _torch():
    import torch

    return torch


_VERSION = operator.attrgetter('_version')


class GcColumn(ctypes.Structure):
    _fields_ = [
        ('src', ctypes.c_void_p),
        ('dst', ctypes.c_void_p),
        ('row_bytes', ctypes.c_int64),
        ('select', ctypes.c_int32),
        ('src_stride', ctypes.c_int32),
    ]


def periodic_layout(num_rows, valid, ends):
    """(period, picks per period, trajectory-end offset) when the buffer is a
    run of equal trajectories -- the OGBench layout: every episode the same
    length, its last row invalid -- else (0, 0, 0).  ``valid``: valid_idxs or
    None (every row pickable); ``ends``: the trajectory end of every pick.
    The kernels then compute a pick's row and trajectory end instead of
    loading them (``ogbx_gc_buffer.period``).  Accepted only if the closed
    form equals ``valid`` and ``ends`` for every pick (checked where the
    tensors live), so the samples are identical either way."""
    torch = _torch()
    R = int(num_rows)
    if valid is not None:
        V = valid.numel()
        ntraj = R - V  # one invalid row per trajectory
        if ntraj <= 0 or R % ntraj or V % ntraj:
            return (0, 0, 0)
        P, pp = R // ntraj, V // ntraj
    else:
        if ends.numel() != R:
            return (0, 0, 0)
        P = int(ends[0]) + 1
        if R % P:
            return (0, 0, 0)
        pp = P
    E = int(ends[0])
    if not 0 <= E < P:
        return (0, 0, 0)
    k = torch.arange(ends.numel(), dtype=torch.int64, device=ends.device)
    q = torch.div(k, pp, rounding_mode='floor')
    if valid is not None and not torch.equal(q * P + (k - q * pp), valid):
        return (0, 0, 0)
    if not torch.equal(q * P + E, ends):
        return (0, 0, 0)
    return (P, pp, E)


class GcBuffer(ctypes.Structure):
    _fields_ = [
        ('num_rows', ctypes.c_int64),
        ('valid_idxs', ctypes.c_void_p),
        ('num_valid', ctypes.c_int64),
        ('traj_end', ctypes.c_void_p),
        ('valid_traj_end', ctypes.c_void_p),
        ('valid_pairs', ctypes.c_void_p),
        ('period', ctypes.c_int64),
        ('period_picks', ctypes.c_int64),
        ('period_end', ctypes.c_int64),
    ]


class GcConfig(ctypes.Structure):
    _fields_ = [
        ('value_p_curgoal', ctypes.c_double),
        ('value_traj_thresh', ctypes.c_double),
        ('value_discount', ctypes.c_double),
        ('actor_p_curgoal', ctypes.c_double),
        ('actor_traj_thresh', ctypes.c_double),
        ('actor_discount', ctypes.c_double),
        ('value_geom_sample', ctypes.c_int32),
        ('actor_geom_sample', ctypes.c_int32),
        ('value_cur_is_one', ctypes.c_int32),
        ('actor_cur_is_one', ctypes.c_int32),
        ('gc_negative', ctypes.c_int32),
        ('pad_', ctypes.c_int32),
    ]


_DRAW_INT = ('pick', 'v_pick', 'v_geom', 'a_pick', 'a_geom')
_DRAW_FLOAT = ('v_dist', 'v_u_traj', 'v_u_cur', 'a_dist', 'a_u_traj', 'a_u_cur')
_DRAW_ORDER = ('pick', 'v_pick', 'v_geom', 'v_dist', 'v_u_traj', 'v_u_cur',
               'a_pick', 'a_geom', 'a_dist', 'a_u_traj', 'a_u_cur')
# HGCDataset's low-level value goal draws
_HDRAW_LOW = ('l_pick', 'l_geom', 'l_u_traj', 'l_u_cur')
_HDRAW_INT = _DRAW_INT + ('l_pick', 'l_geom')


class GcDraws(ctypes.Structure):
    _fields_ = [('idxs', ctypes.c_void_p)] + [(k, ctypes.c_void_p) for k in _DRAW_ORDER]


class GcDrawRecord(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _DRAW_ORDER]


class VisualColumn(ctypes.Structure):
    _fields_ = [
        ('src', ctypes.c_void_p),
        ('dst', ctypes.c_void_p),
        ('height', ctypes.c_int32),
        ('width', ctypes.c_int32),
        ('px_bytes', ctypes.c_int32),
        ('select', ctypes.c_int32),
        ('stack', ctypes.c_int32),
        ('crop', ctypes.c_int32),
    ]


class VisualIndices(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('idxs', 'value_goal_idxs', 'actor_goal_idxs', 'low_value_goal_idxs')]


CROP_PADDING = 3  # GCDataset.augment (datasets.py:331)

# the agents whose GCDataset batches carry the value-midpoint keys (datasets.py:198, 254)
TRL_AGENTS = ('trl', 'latent_trl', 'discrete_latent_trl')
_TRL_SCALARS = ('idxs', 'value_goal_idxs', 'actor_goal_idxs', 'value_midpoint_idxs', 'value_offsets',
                'value_midpoint_offsets', 'masks', 'rewards', 'bad_count')
# the observation-valued keys of the TRL branch, all in its augment list (datasets.py:283-290)
_TRL_IMAGE_KEYS = ('value_goal_observations', 'actor_goal_observations', 'value_midpoint_observations',
                   'value_midpoint_goals', 'value_cur_goals', 'value_next_goals')
TRL_SELECT_MIDPOINT = 4  # OGBX_TRL_SELECT_MIDPOINT
# any other setting lets a value goal fall on or before its sample, where the
# reference fails by its assert or by randint(low >= high)
_TRL_VALUE_GOALS = ('a TRL agent needs value_p_curgoal == 0 and value_p_randomgoal == 0 '
                    '(the value goal must lie past the sample in its trajectory)')


class TrlOutputs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _TRL_SCALARS]


# What a TRL batch holds after the data's own keys, in the reference's order
# (datasets.py:228-276), in the style of ``_HGC_LAYOUT``: (key, source, select)
# is a gathered column, its source 'goal' being ``oracle_reps`` where the data
# has it and ``observations`` otherwise; (key, 'scalar', dtype) a per-sample
# output of the kernel.  Keys with one (source, select) share one tensor
# (``_SamplerHost._trl_walk``).
_TRL_LAYOUT = (
    ('value_goals', 'goal', 2),
    ('actor_goals', 'goal', 3),
    ('masks', 'scalar', 'float64'),
    ('rewards', 'scalar', 'float64'),
    ('value_goal_observations', 'observations', 2),
    ('actor_goal_observations', 'observations', 2),  # the value goal, as the reference (datasets.py:262)
    ('value_offsets', 'scalar', 'int64'),
    ('value_midpoint_offsets', 'scalar', 'int64'),
    ('value_midpoint_observations', 'observations', TRL_SELECT_MIDPOINT),
    ('value_midpoint_actions', 'actions', TRL_SELECT_MIDPOINT),
    ('next_actions', 'actions', 1),  # the data's actions[idxs + 1]
    ('value_midpoint_goals', 'goal', TRL_SELECT_MIDPOINT),
    ('value_cur_goals', 'goal', 0),
    ('value_next_goals', 'goal', 1),  # the data's row idxs + 1, not a stored next_observations
)


ATC_CROP_PADDING = 4  # ATCDataset.augment's default augment_padding (datasets.py:440)


class AtcColumn(ctypes.Structure):
    _fields_ = [
        ('src', ctypes.c_void_p),
        ('anchor', ctypes.c_void_p),
        ('positive', ctypes.c_void_p),
        ('height', ctypes.c_int32),
        ('width', ctypes.c_int32),
        ('px_bytes', ctypes.c_int32),
        ('crop', ctypes.c_int32),
    ]


class AtcOutputs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('idxs', 'pick', 'crop_from', 'bad_count')]


class ReplayInsertColumn(ctypes.Structure):
    _fields_ = [
        ('dst', ctypes.c_void_p),
        ('src', ctypes.c_void_p),
        ('alt', ctypes.c_void_p),
        ('row_elems', ctypes.c_int64),
        ('src_dtype', ctypes.c_int32),
        ('dst_dtype', ctypes.c_int32),
        ('op', ctypes.c_int32),
        ('pad_', ctypes.c_int32),
    ]


REPLAY_MAX_COLS = 16  # OGBX_REPLAY_MAX_COLS
REPLAY_OP_NONE, REPLAY_OP_ONE_MINUS = 0, 1  # ogbx_replay_op


class OnlineRing(ctypes.Structure):
    """ogbx_online_ring (include/ogbx_online.h)."""
    _fields_ = [
        ('num_envs', ctypes.c_int64),
        ('horizon', ctypes.c_int64),
        ('steps', ctypes.c_int64),
        ('ep_seq', ctypes.c_void_p),
        ('cur_seq', ctypes.c_void_p),
        ('ep_end', ctypes.c_void_p),
    ]


class OnlineBatch(ctypes.Structure):
    """ogbx_online_batch (include/ogbx_online.h)."""
    _fields_ = [
        ('cols', ctypes.c_void_p),
        ('num_cols', ctypes.c_int32),
        ('pad_', ctypes.c_int32),
        ('total', ctypes.c_int64),
        ('idxs_out', ctypes.c_void_p),
        ('value_goal_out', ctypes.c_void_p),
        ('actor_goal_out', ctypes.c_void_p),
        ('masks', ctypes.c_void_p),
        ('rewards', ctypes.c_void_p),
    ]


def _bind():
    L = _lib.lib()
    if not getattr(L, '_gc_bound', False):
        P = ctypes.POINTER
        L.ogbx_gc_sample.restype = ctypes.c_int32
        L.ogbx_gc_sample.argtypes = [
            P(GcBuffer), P(GcConfig), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
            P(GcDraws), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, P(GcDrawRecord), ctypes.c_void_p,
        ]
        L.ogbx_gc_sample_ahead.restype = ctypes.c_int32
        L.ogbx_gc_sample_ahead.argtypes = [
            P(GcBuffer), P(GcConfig), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ]
        L.ogbx_gc_plan_create.restype = ctypes.c_int32
        L.ogbx_gc_plan_create.argtypes = [P(GcBuffer), P(GcConfig), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32,
                                          P(ctypes.c_void_p)]
        L.ogbx_gc_plan_set_batch.restype = ctypes.c_int32
        L.ogbx_gc_plan_set_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ogbx_gc_plan_sample.restype = ctypes.c_int32
        L.ogbx_gc_plan_sample.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p]
        L.ogbx_gc_plan_hits.restype = ctypes.c_int64
        L.ogbx_gc_plan_hits.argtypes = [ctypes.c_void_p]
        L.ogbx_gc_plan_destroy.restype = ctypes.c_int32
        L.ogbx_gc_plan_destroy.argtypes = [ctypes.c_void_p]
        L.ogbx_gc_traj_end.restype = ctypes.c_int32
        L.ogbx_gc_traj_end.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_void_p]
        L.ogbx_nonzero_f32.restype = ctypes.c_int32
        L.ogbx_nonzero_f32.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]
        # include/ogbx_visual.h (its own header and version; not part of ogbx.h)
        L.ogbx_visual_api_version.restype = ctypes.c_int32
        L.ogbx_visual_api_version.argtypes = []
        L.ogbx_visual_gather.restype = ctypes.c_int32
        L.ogbx_visual_gather.argtypes = [
            P(GcBuffer), P(HgcConfig), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, P(VisualIndices),
            ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
            ctypes.c_void_p, ctypes.c_void_p,
        ]
        # include/ogbx_trl.h (likewise its own header and version)
        L.ogbx_trl_api_version.restype = ctypes.c_int32
        L.ogbx_trl_api_version.argtypes = []
        L.ogbx_trl_sample.restype = ctypes.c_int32
        L.ogbx_trl_sample.argtypes = [
            P(GcBuffer), P(GcConfig), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, P(GcDraws),
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, P(TrlOutputs), P(GcDrawRecord), ctypes.c_void_p,
            ctypes.c_void_p,
        ]
        L.ogbx_trl_valid_idxs.restype = ctypes.c_int32
        L.ogbx_trl_valid_idxs.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]
        # include/ogbx_atc.h (likewise)
        L.ogbx_atc_api_version.restype = ctypes.c_int32
        L.ogbx_atc_api_version.argtypes = []
        L.ogbx_atc_valid_idxs.restype = ctypes.c_int32
        L.ogbx_atc_valid_idxs.argtypes = [P(GcBuffer), ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]
        L.ogbx_atc_sample.restype = ctypes.c_int32
        L.ogbx_atc_sample.argtypes = [
            P(GcBuffer), P(AtcColumn), ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
            ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
            ctypes.c_uint64, ctypes.c_uint64, P(AtcOutputs), ctypes.c_void_p,
        ]
        # include/ogbx_replay.h (likewise)
        L.ogbx_replay_api_version.restype = ctypes.c_int32
        L.ogbx_replay_api_version.argtypes = []
        L.ogbx_replay_insert.restype = ctypes.c_int32
        L.ogbx_replay_insert.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]
        L.ogbx_replay_clear.restype = ctypes.c_int32
        L.ogbx_replay_clear.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.ogbx_replay_sample.restype = ctypes.c_int32
        L.ogbx_replay_sample.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        # include/ogbx_online.h (likewise)
        L.ogbx_online_api_version.restype = ctypes.c_int32
        L.ogbx_online_api_version.argtypes = []
        L.ogbx_online_insert.restype = ctypes.c_int32
        L.ogbx_online_insert.argtypes = [P(OnlineRing), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]
        L.ogbx_online_clear.restype = ctypes.c_int32
        L.ogbx_online_clear.argtypes = [P(OnlineRing), ctypes.c_void_p]
        L.ogbx_online_gc_sample.restype = ctypes.c_int32
        L.ogbx_online_gc_sample.argtypes = [P(OnlineRing), P(GcConfig), P(OnlineBatch), P(GcDraws), P(GcDrawRecord),
                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        # include/ogbx_online_hgc.h (likewise)
        L.ogbx_online_hgc_api_version.restype = ctypes.c_int32
        L.ogbx_online_hgc_api_version.argtypes = []
        L.ogbx_online_hgc_sample.restype = ctypes.c_int32
        L.ogbx_online_hgc_sample.argtypes = [P(OnlineRing), P(GcConfig), P(HgcConfig), ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_int64, P(HgcDraws), P(HgcOutputs), P(HgcDrawRecord),
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        L._gc_bound = True
    return L


def nonzero_positive(x):
    """nonzero(x > 0) of a float32 device vector, via the libogbx compaction."""
    torch = _torch()
    x = x.reshape(-1)
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    x = x.contiguous()
    L = _bind()
    out = torch.empty(x.numel(), dtype=torch.int64, device=x.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=x.device)
    _lib.check(L.ogbx_nonzero_f32(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.ptr(cnt),
                                  _lib.stream_of(x.device)))
    return out[: int(cnt.item())]


def _to_device(v, device):
    torch = _torch()
    if isinstance(v, torch.Tensor):
        t = v.to(device)
    else:
        t = torch.as_tensor(np.ascontiguousarray(v), device=device)
    return t.contiguous()


class Dataset(dict):
    """Dataset of device tensors (reference: datasets.py:36-83).

    Keys are kept in insertion order; arrays are moved to ``device`` once
    (HBM-resident).  ``valid_idxs`` is computed on the device when 'valids'
    exists (datasets.py:59-60).
    """

    @classmethod
    def create(cls, freeze=True, device=None, **fields):
        assert 'observations' in fields
        return cls(fields, device=device)

    def __init__(self, data=(), device=None, **kw):
        torch = _torch()
        data = dict(data, **kw)
        if device is None:
            first = next(iter(data.values()))
            device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else 'cuda'
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        super().__init__({k: _to_device(v, self.device) for k, v in data.items()})
        self.size = max(len(v) for v in self.values())
        if 'valids' in self:
            self.valid_idxs = nonzero_positive(self['valids'])
        self._seed = None
        self._calls = 0

    # column replacements bump _gen, so that a sampler's per-call staleness
    # check is one int compare plus the packed columns' version counters
    _gen = 0

    def __setitem__(self, key, value):
        self._gen += 1
        super().__setitem__(key, value)

    def __delitem__(self, key):
        self._gen += 1
        super().__delitem__(key)

    def update(self, *a, **kw):
        self._gen += 1
        super().update(*a, **kw)

    def pop(self, *a):
        self._gen += 1
        return super().pop(*a)

    def popitem(self):
        self._gen += 1
        return super().popitem()

    def clear(self):
        self._gen += 1
        super().clear()

    def setdefault(self, key, default=None):
        self._gen += 1
        return super().setdefault(key, default)

    def __ior__(self, other):
        self._gen += 1
        return super().__ior__(other)

    def copy(self, add_or_replace=None):
        d = dict(self)
        if add_or_replace:
            d.update(add_or_replace)
        return Dataset(d, device=self.device)

    # the sampling entry points go through GCDataset's kernel with both goal
    # relabels disabled (p_curgoal = 1 short-circuit, datasets.py:318-319)
    def _sampler(self):
        if getattr(self, '_plain_sampler', None) is None:
            self._plain_sampler = GCDataset(self, _PLAIN_CONFIG, _plain=True)
        return self._plain_sampler

    def get_random_idxs(self, num_idxs):
        """datasets.py:65-70 (Philox draws on the device)."""
        return self._sampler().sample(num_idxs, _keys=())['_idxs']

    def sample(self, batch_size, idxs=None):
        out = self._sampler().sample(batch_size, idxs=idxs)
        for k in ('value_goals', 'actor_goals', 'masks', 'rewards', '_idxs'):
            out.pop(k, None)
        return out

    def get_subset(self, idxs):
        return self.sample(len(idxs), idxs=idxs)


_PLAIN_CONFIG = dict(
    discount=0.99, value_p_curgoal=1.0, value_p_trajgoal=0.0, value_p_randomgoal=0.0, value_geom_sample=False,
    actor_p_curgoal=1.0, actor_p_trajgoal=0.0, actor_p_randomgoal=0.0, actor_geom_sample=False,
    gc_negative=False, p_aug=None, frame_stack=None,
)


def _gc_config(c):
    """ogbx_gc_config of a GCDataset config dict."""

    def thresh(p_traj, p_cur):
        return p_traj / (1.0 - p_cur) if p_cur != 1.0 else 0.0  # datasets.py:321

    return GcConfig(
        float(c['value_p_curgoal']), thresh(c['value_p_trajgoal'], c['value_p_curgoal']), float(c['discount']),
        float(c['actor_p_curgoal']), thresh(c['actor_p_trajgoal'], c['actor_p_curgoal']), float(c['discount']),
        int(bool(c['value_geom_sample'])), int(bool(c['actor_geom_sample'])),
        int(c['value_p_curgoal'] == 1.0), int(c['actor_p_curgoal'] == 1.0), int(bool(c['gc_negative'])), 0,
    )


def _visual_config(config, data):
    """(frame_stack or None, p_aug, p_aug live?, visual?) of a sampler over
    ``data``, for GCDataset and its subclasses and for the ring buffers.

    The p_aug rule of every sample() path: one np.random.rand() per call when
    p_aug > 0 and not evaluation, else none.  The reference draws whenever
    p_aug is not None (impls/utils/datasets.py:278); with p_aug <= 0 its test
    can never pass and the draw would only advance numpy's global stream
    (which the samplers' Philox draws do not follow), so it is skipped.
    visual: some column is stacked or may be cropped (4-D observations)."""
    fs = config.get('frame_stack')
    frame_stack = int(fs) if fs is not None else None
    if fs is not None:
        assert 1 <= frame_stack <= 8 and data['observations'].dim() >= 2
    p_aug = config.get('p_aug')
    live = p_aug is not None and float(p_aug) > 0.0
    visual = fs is not None or (live and any(
        data[k].dim() == 4 for k in ('observations', 'next_observations') if k in data))
    return frame_stack, p_aug, live, visual


class _CallHost:
    """What every sampler keeps per call: the ``(seed, call)`` counter of its
    Philox stream and the ``out=`` caches."""

    def _next_seed(self):
        if self._seed is None:
            self._seed = int(np.random.randint(0, 2**63 - 1))
        call = self._calls
        self._calls += 1
        return self._seed, call

    # An out= cache: the last two batches that plain calls returned, by
    # id(out), each with its shape and what a refill passes on.  A steady
    # refill is host-bound, so the lookup and the refill's
    # one ctypes call stand in line in each sample(), not behind a call of
    # their own; only a new batch comes through here.
    @staticmethod
    def _remember(cache, out, shape, *held):
        if len(cache) >= 2:
            cache.clear()
        cache[id(out)] = (out, shape, *held)

    # Only an injected array comes through the two below: an out= refill has none.
    def _stage_flat(self, v, total, what):
        """An explicit array of ``total`` rows or draws as a flat int64 device tensor."""
        t = _to_device(v, self.device).to(_torch().int64).reshape(-1)
        if t.numel() != total:
            raise ValueError(f'{what} must have {total} entries, got {t.numel()}')
        return t

    def _stage_crop_from(self, crop_from, total):
        """Injected crop offsets as the [total, 2] int64 device tensor."""
        cf = _to_device(crop_from, self.device).to(_torch().int64)
        if tuple(cf.shape) != (total, 2):
            raise ValueError(f"draws['crop_from'] must have shape ({total}, 2), got {tuple(cf.shape)}")
        return cf


class _SamplerHost(_CallHost):
    """The host side of goal-conditioned sampling that the dataset samplers
    (``GCDataset``, ``HGCDataset``) and the ring buffers (``GCReplayBuffer``,
    ``HGCReplayBuffer``) share: staging of explicit idxs and injected draws,
    the draw hooks, the crop coin and the midpoint draw, the walks that lay a
    GC and a TRL batch out, the image geometry of a visual column, the
    bad-sample readback and the ``_*`` keys of a recording call.

    A family supplies ``dataset`` (the columns, by key), ``device``, what
    ``_visual_config`` returned (``_frame_stack``, ``_p_aug``, ``_p_aug_live``,
    ``_visual``), ``_gather`` -- where a column comes from -- with
    ``_VisualColumn``, its entry points (``_direct`` / ``_sample_entry``) and
    its own ``out=`` caches and staleness test.  ``_HgcHost`` overrides the
    hooks of the hierarchical samplers."""

    # the keys a visual sampler may stack, and of those the ones augment() crops
    _VISUAL_KEYS = ('observations', 'next_observations', 'value_goals', 'actor_goals')
    _CROP_KEYS = _VISUAL_KEYS
    _TRL_OK = True  # the reference's GCDataset.sample has the TRL branch; HGCDataset.sample has none
    _draw_keys = _DRAW_ORDER  # the draws a call takes and a recording call reports
    _strict_draws = True  # a draw the sampler does not take raises ValueError (GCDataset: is skipped)
    _trl_bad = None  # where an unchecked TRL call counts its bad samples (the ring's device counter)

    # ------------------------------------------------------------ draws, staging
    def _draw_structs(self):
        """(injected draws to fill, its GC part)."""
        dr = GcDraws()
        return dr, dr

    def _record_struct(self, rec_t):
        return GcDrawRecord(*[rec_t[k].data_ptr() for k in _DRAW_ORDER])

    def _stage(self, total, idxs, draws, record_draws):
        """Explicit idxs and injected draws on the device and the record
        buffers of a recording call: (draws struct, or None when nothing is
        injected; tensors to keep alive until the launch was issued; record
        struct or None; its tensors or None).  A wrong length raises
        ValueError, and so does a draw the sampler does not take
        (``_strict_draws``)."""
        torch = _torch()
        dr = rec = rec_t = None
        staged = []
        if idxs is not None or draws:
            dr, gdr = self._draw_structs()
            if idxs is not None:
                t = self._stage_flat(idxs, total, 'idxs')
                staged.append(t)
                gdr.idxs = t.data_ptr()
            for k, v in (draws or {}).items():
                if k == 'idxs':
                    continue
                if k not in self._draw_keys:
                    if self._strict_draws:
                        raise ValueError(f'unknown draw {k!r}')
                    continue
                t = _to_device(v, self.device).to(torch.int64 if k in _HDRAW_INT else torch.float64).reshape(-1)
                if t.numel() != total:
                    raise ValueError(f'draw {k!r} must have {total} entries, got {t.numel()}')
                staged.append(t)
                setattr(dr if k in _HDRAW_LOW else gdr, k, t.data_ptr())
        if record_draws:
            rec_t = {k: torch.empty(total, dtype=torch.int64 if k in _HDRAW_INT else torch.float64,
                                    device=self.device) for k in self._draw_keys}
            rec = self._record_struct(rec_t)
        return dr, staged, rec, rec_t

    # The crop coin (datasets.py:278-279: one np.random.rand() on the host; the
    # offsets are device draws), the pops of 'crop_from' / 'midpoint' and the
    # *checked* rule of a TRL call stand in line in each visual and TRL
    # sample(): an out= refill passes them.  Only an injected draw is staged
    # (``_CallHost._stage_crop_from``, and the midpoint here).
    def _stage_midpoint(self, midpoint, total):
        """Injected midpoint rows as an int64 device tensor of ``total``."""
        return self._stage_flat(midpoint, total, "draws['midpoint']")

    @staticmethod
    def _check_bad(bad, total, what):
        """Read a checked TRL call's counter back and raise on bad samples."""
        n = int(bad.item())
        if n:
            raise ValueError(f'{what}: {n} of {total} samples have no row between the sample and its value goal '
                             f'(an index names the last row of its trajectory, or the injected draws put the value '
                             f'goal at or before the sample)')

    @staticmethod
    def _recorded(rec_t, idx_t, **more):
        """The ``_*`` keys a recording call adds to its batch: the draws used,
        with those of ``more`` the call made, and the index outputs."""
        rec_t.update((k, v) for k, v in more.items() if v is not None)
        return {'_draws': rec_t, **idx_t}

    # ----------------------------------------------------------- image columns
    def _visual_spec(self, src_key, dst_key):
        """(stack, crop) when ``dst_key`` is an image column of this visual
        sampler (written by the visual gather), else None (a fused column)."""
        if not self._visual or dst_key not in self._VISUAL_KEYS:
            return None
        if src_key not in ('observations', 'next_observations'):
            return None  # oracle_reps: neither stacked nor cropped
        stack = self._frame_stack is not None
        crop = self._p_aug_live and self.dataset[src_key].dim() == 4 and dst_key in self._CROP_KEYS
        return (stack, crop) if (stack or crop) else None

    def _image_column(self, src, lead, select, spec, total):
        """Destination tensor and descriptor (``_VisualColumn``, whose leading
        source fields are ``lead``) of one image column over ``src``."""
        stack, crop = spec
        shape = tuple(src.shape[1:])
        F = self._frame_stack if stack else 1
        dst = _torch().empty((total,) + shape[:-1] + (shape[-1] * F,), dtype=src.dtype, device=self.device)
        # an image is [H, W, C]; any other row is a 1-row image of its leading elements
        H, W = (shape[0], shape[1]) if len(shape) == 3 else (1, int(np.prod(shape[:-1], dtype=np.int64)))
        return dst, self._VisualColumn(*lead, dst.data_ptr(), H, W, shape[-1] * src.element_size(), select,
                                       int(stack), int(crop))

    def _hcfg_ptr(self):
        return None  # the hierarchical samplers pass their ogbx_hgc_config

    def _visual_indices(self, idx_t):
        """The fused launch's index outputs as the visual gather reads them."""
        return VisualIndices(idx_t['_idxs'].data_ptr(), idx_t['_value_goal_idxs'].data_ptr(),
                             idx_t['_actor_goal_idxs'].data_ptr(), None)

    # ------------------------------------------------------------ batch layouts
    def _own_columns(self):
        """(source key, batch key, selector) of the data's own keys."""
        return [(k, k, 0) for k in self.dataset]

    def _goal_source(self):
        return 'oracle_reps' if 'oracle_reps' in self.dataset else 'observations'  # datasets.py:348-357

    def _gc_walk(self, total, vcols=None):
        """The gathered keys of a GC batch in the reference's order, and the
        fused columns' descriptors (image columns go to ``vcols``)."""
        out, cols = {}, []
        for src_key, key, select in self._own_columns():
            out[key] = self._gather(src_key, key, select, total, cols, vcols)
        goal_src = self._goal_source()
        for key, select in (('value_goals', 2), ('actor_goals', 3)):
            out[key] = self._gather(goal_src, key, select, total, cols, vcols)
        return out, cols

    def _trl_walk(self, total, record, checked, vcols=None, mcols=None):
        """A new TRL batch: the data's own keys, then ``_TRL_LAYOUT``.  Each
        distinct (source, selector) is gathered once; keys the reference
        computes by the same expression share the tensor.  Image columns go to
        ``vcols``, those selected through the midpoint to ``mcols``.  Returns
        the batch, the fused columns' descriptors, ``TrlOutputs``, the index
        outputs -- there only when something reads them, the gathers of a
        visual batch or a recording call -- and the bad-sample counter of a
        checked call (else None: ``_trl_bad`` counts)."""
        torch = _torch()
        out, cols, made = {}, [], {}
        goal_src = self._goal_source()

        # ``made`` is keyed by (source, selector) alone: every observation-valued
        # key of the layout is an image key of a visual TRL sampler, so whether
        # a column is stacked or cropped depends on its source only
        assert vcols is None or all(k in self._CROP_KEYS for k, what, _ in _TRL_LAYOUT
                                    if what in ('observations', 'goal'))

        def add(src_key, key, select):
            dst = made.get((src_key, select))
            if dst is None:
                mid = mcols is not None and select == TRL_SELECT_MIDPOINT
                n = len(mcols) if mid else 0
                dst = made[(src_key, select)] = self._gather(src_key, key, select, total, cols,
                                                             mcols if mid else vcols)
                if mid and len(mcols) > n:
                    # the midpoint's image columns go to a gather of their own,
                    # which reads value_midpoint_idxs as its idxs (selector 0)
                    mcols[-1].select = 0
            out[key] = dst

        for src_key, key, select in self._own_columns():
            add(src_key, key, select)
        for key, what, arg in _TRL_LAYOUT:
            if what == 'scalar':
                out[key] = torch.empty(total, dtype=getattr(torch, arg), device=self.device)
            else:
                add(goal_src if what == 'goal' else what, key, arg)
        idx_t = {'_' + k: torch.empty(total, dtype=torch.int64, device=self.device)
                 for k in (_TRL_SCALARS[:4] if (record or vcols is not None) else ())}
        bad = torch.zeros(1, dtype=torch.int64, device=self.device) if checked else None
        outs = TrlOutputs(*[_lib.ptr(idx_t.get('_' + k)) for k in _TRL_SCALARS[:4]],
                          *[out[k].data_ptr() for k in _TRL_SCALARS[4:8]],
                          _lib.ptr(bad if checked else self._trl_bad))
        return out, cols, outs, idx_t, bad


class GCDataset(_SamplerHost):
    """Goal-conditioned sampler (reference: datasets.py:149-366).

    config keys read (as the reference): discount, value_/actor_ p_curgoal,
    p_trajgoal, p_randomgoal, geom_sample, gc_negative, p_aug, frame_stack;
    and two of this sampler's own: row_record (default True; False skips the
    interleaved copy of the small columns, ``_row_record``) and lookahead
    (default True: each plain call of <= 1,024 samples also computes the next
    call's selectors, so the next call only gathers; ``ogbx_gc_plan_*``).

    ``sampler.dataset`` may be reassigned and its columns replaced or modified
    in place: sample() notices (one staleness token, ``_refresh_record``) and
    batches show the current values.  The trajectory tables (``_buf``,
    ``traj_end``, ``valid_idxs``) are fixed at construction, as the
    reference's ``__post_init__`` fixes its own: a new dataset must keep the
    trajectory layout.

    Visual samplers.  With ``frame_stack = F`` the keys the reference builds
    through get_observations / get_goal_observations (``observations``,
    ``next_observations`` and, without ``oracle_reps``, ``value_goals`` /
    ``actor_goals``) hold F frames stacked on the last axis: channel block j
    is the frame at row max(r - (F-1-j), first row of r's trajectory)
    (datasets.py:359-366).  ``next_observations`` selects min(idx + 1, R - 1);
    the reference indexes idx + 1 unclamped and would raise on the last row,
    which valid rows never reach.  ``frame_stack`` needs a compact dataset (no
    'next_observations') and also stacks 2-D state observations
    ([R, D] -> [B, F D]).  ``preprocess_frame_stack`` is accepted and has no
    effect: the reference's two settings give identical batches, and here the
    frames always stay unstacked in HBM (a third of the memory at F = 3), so
    ``sampler.dataset['observations']`` stays unstacked too.  With
    ``p_aug > 0`` and 4-D observations, a call whose coin comes up (one
    ``np.random.rand()`` per call, not under ``evaluation``) crops those keys
    with padding 3 and one offset pair per sample drawn on the device
    (datasets.py:17-33, 329-339); this also works without ``frame_stack`` and
    on a non-compact dataset.  A visual sampler runs the fused launch over its
    other columns and one ``ogbx_visual_gather`` launch over the image ones;
    it does not use the look-ahead plan.  Its non-image keys and indices are
    those of the same sampler without ``frame_stack`` / ``p_aug`` at the same
    seed and call.

    TRL samplers.  With ``config['agent_name']`` in ``TRL_AGENTS`` a batch
    also carries the keys of the reference's TRL branch (datasets.py:254-276),
    built around the *value midpoint*, a row drawn uniformly in
    [idx, value goal): ``value_goal_observations``, ``actor_goal_observations``
    (both at the value goal, as the reference), ``value_offsets``,
    ``value_midpoint_offsets`` (int64), ``value_midpoint_observations``,
    ``value_midpoint_actions``, ``next_actions``, ``value_midpoint_goals``,
    ``value_cur_goals`` and ``value_next_goals``, in the reference's order.
    One launch of ``trl_sample_kernel`` (``ogbx_trl_sample``,
    include/ogbx_trl.h) draws and gathers all of it; there is no look-ahead
    plan for it.  ``idxs``, the goals, ``masks``, ``rewards`` and the nine GC
    keys are those of a non-TRL sampler over the same pick table at the same
    seed and call.  The config needs ``value_p_curgoal == 0`` and
    ``value_p_randomgoal == 0`` (ValueError otherwise: the reference then
    fails data-dependently, by its assert or by ``randint(low >= high)``).
    Differences from the reference, both deliberate:

    * the pick table -- every row but the last of its trajectory, whether or
      not the dataset has 'valids' (datasets.py:198-204) -- is the sampler's
      own (``_valid``); the reference overwrites ``dataset.valid_idxs``, here
      the shared ``Dataset`` is left as it was;
    * keys the reference computes by the same expression hold ONE tensor, and
      each distinct (source, selector) is gathered once:
      ``actor_goal_observations is value_goal_observations``; without
      ``oracle_reps`` also ``value_cur_goals is observations``,
      ``value_next_goals is next_observations`` (compact datasets; a regular
      one stores its own ``next_observations``),
      ``value_midpoint_goals is value_midpoint_observations`` and
      ``value_goal_observations is value_goals``; with ``oracle_reps``,
      ``value_goals`` (representations) and ``value_goal_observations``
      (observations) are distinct and ``value_cur_goals is oracle_reps``.

    ``next_actions`` / ``value_next_goals`` select min(idx + 1, R - 1), which is
    idx + 1 for every pickable row.  Explicit ``idxs`` that name a
    trajectory's last row (or injected draws with a value goal at or before
    the sample) raise ValueError with the count of such samples, read back
    after the launch; the Philox path reads nothing back.  ``draws`` takes
    ``'midpoint'`` (the rows of the reference's ``randint(idxs,
    value_goal_idxs)``), ``record_draws`` reports it with
    ``_value_midpoint_idxs``.  A visual TRL sampler runs the fused launch, one
    ``ogbx_visual_gather`` over the image columns at idx / next / goals and one
    over those at the midpoint, which share the sample's crop offsets; the six
    observation-valued TRL keys are stacked and cropped like
    ``observations`` unless they come from ``oracle_reps``.
    """

    _VisualColumn = VisualColumn  # ogbx_visual_gather's descriptor
    # the dataset samplers skip a draw they do not take: the fixtures recorded
    # from the reference hand HGCDataset every draw the reference made, among
    # them an 'l_dist' that no kernel reads (tests/golden/hgc_golden.npz)
    _strict_draws = False

    def __init__(self, dataset, config, preprocess_frame_stack=True, seed=None, _plain=False):
        torch = _torch()
        if not isinstance(dataset, Dataset):
            dataset = Dataset(dataset)
        self.dataset = dataset
        self.config = config
        self.preprocess_frame_stack = preprocess_frame_stack
        self.size = dataset.size
        self.device = dataset.device
        if config.get('frame_stack') is not None:
            # only compact (observation-only) datasets (datasets.py:206-208)
            assert 'next_observations' not in dataset
        self._frame_stack, self._p_aug, self._p_aug_live, visual = _visual_config(config, dataset)
        self._visual = visual and not _plain
        self._trl = not _plain and config.get('agent_name') in TRL_AGENTS
        if self._trl:
            if not self._TRL_OK:
                raise NotImplementedError(f'{type(self).__name__}.sample has no TRL branch (nor has the reference)')
            if config['value_p_curgoal'] != 0 or config['value_p_randomgoal'] != 0:
                raise ValueError(_TRL_VALUE_GOALS)
            self._VISUAL_KEYS = self._CROP_KEYS = type(self)._VISUAL_KEYS + _TRL_IMAGE_KEYS
            # a TRL sampler's sample() is bound here, on the instance, and not
            # tested for inside sample(): a steady GC / HGC refill is bounded by
            # host time, and one more attribute test per call measured 12 ns of
            # HGCDataset.sample(1024)'s 6.40 us (profiles/trl_sampler.json,
            # earlier_parent_comparisons.first_attempt)
            self.sample = self._sample_trl_call
        L = _bind()
        self._L = L
        stream = _lib.stream_of(self.device)
        if 'terminals' in dataset:
            self.terminal_locs = nonzero_positive(dataset['terminals'])
        else:
            self.terminal_locs = torch.tensor([self.size - 1], dtype=torch.int64, device=self.device)
        if not _plain:
            assert self.terminal_locs.numel() > 0 and int(self.terminal_locs[-1]) == self.size - 1
            assert np.isclose(
                config['value_p_curgoal'] + config['value_p_trajgoal'] + config['value_p_randomgoal'], 1.0)
            assert np.isclose(
                config['actor_p_curgoal'] + config['actor_p_trajgoal'] + config['actor_p_randomgoal'], 1.0)
        self.initial_locs = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device),
                                       self.terminal_locs[:-1] + 1])
        self.traj_end = torch.empty(self.size, dtype=torch.int64, device=self.device)
        if self.terminal_locs.numel() > 0:
            _lib.check(L.ogbx_gc_traj_end(_lib.ptr(self.terminal_locs), self.terminal_locs.numel(), self.size,
                                          _lib.ptr(self.traj_end), stream))
        else:
            self.traj_end.fill_(self.size - 1)
        valid = getattr(dataset, 'valid_idxs', None)
        if self._trl:
            # the TRL pick table: every row but the last of its trajectory,
            # with or without 'valids' (datasets.py:198-204); the sampler's
            # own, the shared Dataset keeps its valid_idxs
            valid = self._trl_valid_idxs(stream)
        # trajectory end of every valid row: the drawn index and its end load in parallel
        self.valid_traj_end = self.traj_end[valid].contiguous() if valid is not None else None
        # (index, trajectory end) of every valid row interleaved: one 16-B load per pick
        self.valid_pairs = torch.stack([valid, self.valid_traj_end], 1).contiguous() if valid is not None else None
        self.period = periodic_layout(self.size, valid, self.valid_traj_end if valid is not None else self.traj_end)
        self._buf = GcBuffer(self.size, valid.data_ptr() if valid is not None else None,
                             valid.numel() if valid is not None else 0, self.traj_end.data_ptr(),
                             self.valid_traj_end.data_ptr() if valid is not None else None,
                             self.valid_pairs.data_ptr() if valid is not None else None, *self.period)
        self._valid = valid
        self._plain = _plain
        self._record, self._rec_off, self._rec_stride, self._rec_src = self._row_record(dataset)
        self._rec_index()
        # staleness token, compared at the top of sample(): the dataset object,
        # its generation and (_rec_versions) the packed columns' versions
        self._tok_ds, self._tok_gen = dataset, dataset._gen

        self._cfg = _gc_config(config)
        self._seed = int(seed) if seed is not None else None
        self._calls = 0
        self._out_cache = {}
        # plain (Philox, no idxs / draws / recording) calls go through a sampler
        # plan (ogbx_gc_plan_*): the prepared output batches and the look-ahead
        # state live in libogbx, so a steady call is one lookup and one launch
        self._lookahead = bool(config.get('lookahead', self._LOOKAHEAD_DEFAULT))
        self._vis_cache = {}  # (_p_aug_live, _visual: _visual_config, above)
        self._trl_cache = {}
        self._dev_idx = self.device.index
        self._plan_sample = L.ogbx_gc_plan_sample
        self._raw_stream = torch._C._cuda_getCurrentRawStream  # hipStream_t of the current stream, as an int
        self._plan = None
        self._plan_seed = None
        self._plan_final = None
        self._slot = 0

    # ---------------------------------------------------------------- helpers
    _RECORD_MAX = 128  # one L2 line

    def _row_record(self, ds):
        """The sampler's own interleaved copy of the dataset's small columns
        (every key but the goal sources whose row is 4-byte granular, packed in
        key order while they fit one 128-B line per row, e.g. actions 84 +
        terminals 4 + valids 4 of the humanoid layout): a sample's rows of them
        then come from one line of HBM instead of one line per column.  The row
        stride is the power of two (16..128 B) at or above the packed bytes, so
        a row never straddles a line and the copy costs no more than it must
        (pointmaze: actions 8 + terminals 4 + valids 4 = 16 B per row).  The
        dataset's own tensors (and the returned batch) keep the reference
        shapes.  Not built for the plain Dataset.sample sampler, with fewer
        than two packable columns, or with config['row_record'] = False.

        The reference freezes its dataset (Dataset.create sets the arrays
        read-only, impls/utils/datasets.py:45-56); torch tensors cannot be made
        read-only, so sample() checks the packed columns' version counters
        and identities and refreshes the copy if one was modified
        (``_refresh_record``)."""
        torch = _torch()
        if self._plain or not self.config.get('row_record', True):
            return None, {}, 0, ()
        goal_srcs = {'observations', 'oracle_reps'}
        off, picks = 0, []
        for k, v in ds.items():
            if k in goal_srcs:
                continue
            rb = (v[0].numel() if v.dim() > 1 else 1) * v.element_size()
            if rb % 4 or off + rb > self._RECORD_MAX:
                continue
            picks.append((k, off, rb))
            off += rb
        if len(picks) < 2:
            return None, {}, 0, ()
        stride = 16
        while stride < off:
            stride *= 2
        rec = torch.zeros(self.size, stride, dtype=torch.uint8, device=self.device)
        src = tuple((k, ds[k], o, rb) for k, o, rb in picks)
        self._fill_record(rec, src)
        return rec, {k: o for k, o, _ in picks}, stride, tuple((k, t, o, rb, t._version) for k, t, o, rb in src)

    def _fill_record(self, rec, src):
        torch = _torch()
        for k, t, o, rb in src:
            rec[:, o:o + rb] = t.reshape(self.size, -1).contiguous().view(torch.uint8)

    def _refresh_record(self):
        """The full staleness check, run by sample() when its token moved.  A
        new dataset object or generation (a column was replaced, packed or
        not) drops the prepared batches: their descriptors hold the old
        columns' pointers.  A packed column that was replaced or modified in
        place is re-packed (same layout, same record buffer)."""
        ds = self.dataset
        if not isinstance(ds, Dataset):
            ds = self.dataset = Dataset(ds)
        if ds is not self._tok_ds or ds._gen != self._tok_gen:
            self._out_cache.clear()
        stale = False
        for k, t, _, _, ver in self._rec_src:
            cur = ds.get(k)
            if cur is not t:
                if cur is None or cur.shape != t.shape or cur.dtype != t.dtype:
                    raise ValueError(f'dataset column {k!r} changed shape or dtype after the sampler was built')
                stale = True
            elif t._version != ver:
                stale = True
        if stale:
            src = tuple((k, ds[k], o, rb) for k, _, o, rb, _ in self._rec_src)
            self._fill_record(self._record, src)
            self._rec_src = tuple((k, t, o, rb, t._version) for k, t, o, rb in src)
            self._rec_index()
        self._tok_ds, self._tok_gen = ds, ds._gen

    def _rec_index(self):
        self._rec_tensors = tuple(e[1] for e in self._rec_src)
        self._rec_versions = tuple(e[4] for e in self._rec_src)

    def _column(self, src_key, dst, select):
        """Descriptor of one gathered column (from the row record when the key
        lives there)."""
        src = self.dataset[src_key]
        row_bytes = src[0].numel() * src.element_size() if src.dim() > 1 else src.element_size()
        o = self._rec_off.get(src_key)
        if o is not None:
            return GcColumn(self._record.data_ptr() + o, dst.data_ptr(), row_bytes, select, self._rec_stride)
        return GcColumn(src.data_ptr(), dst.data_ptr(), row_bytes, select, 0)

    def _gather(self, src_key, dst_key, select, total, cols, vcols):
        """The destination of one output column.  Its descriptor goes to
        ``vcols`` when it is an image column of a visual sampler (``vcols``
        None: no column is), else to ``cols``, the fused launch's, read from
        the row record when the key lives there."""
        src = self.dataset[src_key]
        spec = self._visual_spec(src_key, dst_key) if vcols is not None else None
        if spec is not None:
            dst, vc = self._image_column(src, (src.data_ptr(),), select, spec, total)
            vcols.append(vc)
        else:
            dst = _torch().empty((total,) + tuple(src.shape[1:]), dtype=src.dtype, device=self.device)
            cols.append(self._column(src_key, dst, select))
        return dst

    def _own_columns(self):
        own = super()._own_columns()
        if 'next_observations' not in self.dataset:
            own.append(('observations', 'next_observations', 1))  # datasets.py:81-82
        return own

    def _columns(self, total, keys, vcols=None):
        """Column descriptors and the output dict (reference key order); the
        image columns of a visual sampler go to ``vcols``.  ``keys``: those of
        the dataset's keys to gather and nothing else (``get_random_idxs``)."""
        if keys is None and not self._plain:
            return self._gc_walk(total, vcols)
        out, cols = {}, []
        for src_key, key, select in (self._own_columns() if keys is None else [(k, k, 0) for k in keys]):
            out[key] = self._gather(src_key, key, select, total, cols, vcols)
        return out, cols


    # GC: with the look-ahead actually hitting (round 5), 4.7 vs 5.8 us per
    # B = 1,024 launch back to back (profiles/r05_gcsample_*), so on by
    # default for both samplers
    _LOOKAHEAD_DEFAULT = True

    def _plan_for(self, seed):
        """The sampler plan of this (dataset, config, seed), created on the
        first plain call (the seed is drawn then if none was given)."""
        if self._plan is None or self._plan_seed != seed:
            self._drop_plan()
            L = self._L
            h = ctypes.c_void_p()
            # the plan also takes its device from the buffer (hipPointerGetAttributes)
            with _torch().cuda.device(self.device):
                _lib.check(L.ogbx_gc_plan_create(self._buf, self._cfg, self._hcfg_ptr(), seed, int(self._lookahead),
                                                 ctypes.byref(h)), 'gc_plan_create')
            self._plan, self._plan_seed = h.value, seed
            self._plan_final = weakref.finalize(self, L.ogbx_gc_plan_destroy, h.value)
            self._out_cache.clear()  # their slots belong to the old plan
        return self._plan

    def _drop_plan(self):
        if self._plan_final is not None:
            self._plan_final()
        self._plan, self._plan_final = None, None

    @property
    def ahead_hits(self):
        """Calls served from selectors the previous launch stored (diagnostic)."""
        return int(self._L.ogbx_gc_plan_hits(self._plan)) if self._plan is not None else 0

    def _next_slot(self):
        slot = self._slot
        self._slot = (slot + 1) % 8  # OGBX_GC_PLAN_SLOTS; the out cache holds at most the last two
        return slot

    # ------------------------------------------ what HGCDataset supplies instead
    # (with the hooks of _SamplerHost that _HgcHost overrides)
    _what = 'gc_sample'  # names the call in error messages

    def _batch(self, total, keys, record, vcols=None):
        """A new batch: the output dict, the column descriptors, the scalar
        outputs as ``_set_batch`` / ``_direct`` pass them on, tensors to keep
        alive with the batch, and the index keys of a recording call."""
        torch = _torch()
        out, cols = self._columns(total, keys, vcols)
        masks = torch.empty(total, dtype=torch.float64, device=self.device)
        rewards = torch.empty(total, dtype=torch.float64, device=self.device)
        # index outputs only when asked for (plain sampling or draw recording)
        idx = torch.empty(total, dtype=torch.int64, device=self.device) if (self._plain or record) else None
        vg = torch.empty(total, dtype=torch.int64, device=self.device) if record else None
        ag = torch.empty(total, dtype=torch.int64, device=self.device) if record else None
        if self._plain:
            out['_idxs'] = idx
        else:
            out['masks'] = masks
            out['rewards'] = rewards
        scalars = tuple(map(_lib.ptr, (idx, vg, ag, masks, rewards)))
        return out, cols, scalars, (masks, rewards), {'_idxs': idx, '_value_goal_idxs': vg, '_actor_goal_idxs': ag}

    def _set_batch(self, plan, slot, col_arr, ncols, B, nb, scalars):
        return self._L.ogbx_gc_plan_set_batch(plan, slot, col_arr, ncols, B, nb, *scalars, None)

    def _direct(self, col_arr, ncols, B, nb, dr, seed, call, scalars, rec, stream):
        return self._L.ogbx_gc_sample(self._buf, self._cfg, col_arr, ncols, B, nb, dr, seed, call, *scalars, rec,
                                      stream)

    def sample(self, batch_size, idxs=None, evaluation=False, draws=None, record_draws=False,
               num_batches=1, _keys=None, out=None):
        """GCDataset.sample (datasets.py:213-294) / HGCDataset.sample
        (datasets.py:496-643), one fused launch.

        draws: optional dict of injected reference draws (see ``_DRAW_ORDER``,
        for HGCDataset also the low-level ``l_*`` draws; device or host arrays
        of length num_batches*batch_size).  A visual sampler also takes
        ``'crop_from'``, the [num_batches*batch_size, 2] offsets (cy, cx) of
        augment()'s randint (datasets.py:333), used when the call crops; a TRL
        sampler ``'midpoint'``, the rows of randint(idxs, value_goal_idxs)
        (datasets.py:259).
        record_draws: also return the draws the kernel used (``out['_draws']``;
        with ``'crop_from'`` on a call that cropped, and without it otherwise).
        num_batches > 1: sample that many independent batches in the same launch
        (outputs have a leading num_batches*batch_size dimension).
        out: a batch dict returned by an earlier call with the same batch_size /
        num_batches (and no idxs/draws/record_draws): its tensors are refilled
        in place (stream ordered, so consumers enqueued earlier read the old
        batch) and it is returned.  Skips all per-call allocation.
        """
        if self._visual:
            return self._sample_visual(int(batch_size), int(num_batches), idxs, evaluation, draws, record_draws, out)
        plain_call = idxs is None and not draws and not record_draws and _keys is None
        # the staleness token: the dataset object, its generation (no column
        # replaced) and the packed columns' version counters (none modified in
        # place); anything else takes the full check
        ds = self.dataset
        if (ds is not self._tok_ds or getattr(ds, '_gen', None) != self._tok_gen
                or (self._rec_src and tuple(map(_VERSION, self._rec_tensors)) != self._rec_versions)):
            self._refresh_record()
        # the steady refill: one dict lookup, one ctypes call (host time per
        # call is what bounds sample(1024)'s rate, bench 'extra')
        hit = self._out_cache.get(id(out)) if (out is not None and plain_call) else None
        if (hit is not None and hit[0] is out and hit[1] == (batch_size, num_batches)
                and self._plan_seed == self._seed):
            call = self._calls
            self._calls = call + 1
            st = self._plan_sample(self._plan, hit[2], call, self._raw_stream(self._dev_idx))
            if st:
                _lib.check(st, self._what)
            extra = None
        else:
            out, extra = self._sample_new(int(batch_size), int(num_batches), idxs, draws, record_draws, _keys,
                                          plain_call, (batch_size, num_batches))
        if self._p_aug_live and not evaluation:
            # the coin of datasets.py:278-279; crops apply only to 4-D arrays,
            # and a sampler with 4-D observations is visual (_sample_visual)
            np.random.rand()
        if extra:
            out.update(extra)
        return out

    # ------------------------------------------------------------ visual batches
    def _sample_visual(self, B, nb, idxs, evaluation, draws, record_draws, out):
        """sample() of a visual sampler: the fused direct launch over the
        non-image columns with the index outputs requested, then one
        ogbx_visual_gather launch over the image columns."""
        torch = _torch()
        total = B * nb
        ds = self.dataset
        if (ds is not self._tok_ds or getattr(ds, '_gen', None) != self._tok_gen
                or (self._rec_src and tuple(map(_VERSION, self._rec_tensors)) != self._rec_versions)):
            self._refresh_record()
            self._vis_cache.clear()
        crop = bool(self._p_aug_live and not evaluation and np.random.rand() < self._p_aug)
        draws = dict(draws or {})
        crop_from = draws.pop('crop_from', None)
        cf = self._stage_crop_from(crop_from, total) if (crop and crop_from is not None) else None
        # as in the fused path, only a call without idxs / draws / recording
        # prepares a batch that ``out=`` can refill
        plain_call = idxs is None and not draws and crop_from is None and not record_draws
        hit = self._vis_cache.get(id(out)) if (out is not None and plain_call) else None
        if hit is not None and hit[0] is out and hit[1] == (B, nb):
            st = hit[2]
        else:
            vcols = []
            out, cols, scalars, keep, idx_t = self._batch(total, None, True, vcols)
            col_keep = (GcColumn * max(1, len(cols)))(*cols)
            vcol_keep = (VisualColumn * max(1, len(vcols)))(*vcols)
            st = (ctypes.cast(col_keep, ctypes.c_void_p), len(cols), scalars, ctypes.cast(vcol_keep, ctypes.c_void_p),
                  len(vcols), self._visual_indices(idx_t), idx_t, (col_keep, vcol_keep, keep))
            if plain_call:
                self._remember(self._vis_cache, out, (B, nb), st)
        col_arr, ncols, scalars, vcol_arr, nvcols, vidx, idx_t, _ = st
        dr, staged, rec, rec_t = self._stage(total, idxs, draws, record_draws)
        cf_out = torch.empty((total, 2), dtype=torch.int64, device=self.device) if (crop and record_draws) else None
        seed, call = self._next_seed()
        stream = _lib.stream_of(self.device)
        _lib.check(self._direct(col_arr, ncols, B, nb, dr, seed, call, scalars, rec, stream), self._what)
        _lib.check(self._L.ogbx_visual_gather(
            self._buf, self._hcfg_ptr(), vcol_arr, nvcols, total, vidx, self._frame_stack or 1, CROP_PADDING,
            _lib.ptr(cf), int(crop and cf is None), seed, call, _lib.ptr(cf_out), stream), 'visual_gather')
        del staged, cf  # alive until the launches were issued
        if record_draws:
            out.update(self._recorded(rec_t, idx_t, crop_from=cf_out))
        return out

    # --------------------------------------------------------------- TRL batches
    def _trl_valid_idxs(self, stream):
        """Every row that is not the last of its trajectory, in order
        (datasets.py:198-204), compacted on the device from ``traj_end``."""
        torch = _torch()
        rows = torch.empty(self.size, dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        _lib.check(self._L.ogbx_trl_valid_idxs(_lib.ptr(self.traj_end), self.size, _lib.ptr(rows), _lib.ptr(cnt),
                                               stream), 'trl_valid_idxs')
        return rows[: int(cnt.item())]

    def _trl_batch(self, total, record, checked):
        """A new TRL batch: the output dict in the reference's key order
        (datasets.py:228-276), the descriptors of the fused columns (selectors
        0..4), of the image columns selected through idx / next / goals and of
        those selected through the midpoint, and the scalar outputs.  Each
        distinct (source, selector) is gathered once; keys the reference
        computes by the same expression share the tensor."""
        vcols, mcols = ([], []) if self._visual else (None, None)
        out, cols, outs, idx_t, bad = self._trl_walk(total, record, checked, vcols, mcols)
        vcols, mcols = vcols or (), mcols or ()
        col_keep = (GcColumn * max(1, len(cols)))(*cols)
        vcol_keep = (VisualColumn * max(1, len(vcols)))(*vcols)
        mcol_keep = (VisualColumn * max(1, len(mcols)))(*mcols)
        vidx = midx = None
        if self._visual:
            vidx = self._visual_indices(idx_t)
            midx = VisualIndices(idx_t['_value_midpoint_idxs'].data_ptr(), None, None, None)
        return (out, ctypes.cast(col_keep, ctypes.c_void_p), len(cols), outs,
                ctypes.cast(vcol_keep, ctypes.c_void_p), len(vcols), vidx,
                ctypes.cast(mcol_keep, ctypes.c_void_p), len(mcols), midx, idx_t, bad,
                (col_keep, vcol_keep, mcol_keep))

    def _sample_trl_call(self, batch_size, idxs=None, evaluation=False, draws=None, record_draws=False,
                         num_batches=1, out=None):
        """``sample`` of a TRL sampler (see ``sample`` for the arguments)."""
        return self._sample_trl(int(batch_size), int(num_batches), idxs, evaluation, draws, record_draws, out)

    def _sample_trl(self, B, nb, idxs, evaluation, draws, record_draws, out):
        """sample() of a TRL sampler (datasets.py:213-294 with the branch of
        254-276): one ``trl_sample_kernel`` launch (``ogbx_trl_sample``) over
        the non-image columns; a visual sampler adds one ``ogbx_visual_gather``
        over the image columns selected through idx / next / goals and one over
        those selected through the midpoint (same seed and call, so the same
        crop offsets).  ``draws`` also takes ``'midpoint'``, the rows the
        reference's ``randint(idxs, value_goal_idxs)`` returned."""
        torch = _torch()
        total = B * nb
        ds = self.dataset
        if (ds is not self._tok_ds or getattr(ds, '_gen', None) != self._tok_gen
                or (self._rec_src and tuple(map(_VERSION, self._rec_tensors)) != self._rec_versions)):
            self._refresh_record()
            self._trl_cache.clear()
        # a non-visual sampler crops nothing; its coin is drawn after the launch, below
        crop = bool(self._visual and self._p_aug_live and not evaluation and np.random.rand() < self._p_aug)
        draws = dict(draws or {})
        crop_from = draws.pop('crop_from', None)
        midpoint = draws.pop('midpoint', None)
        cf = self._stage_crop_from(crop_from, total) if (crop and crop_from is not None) else None
        mid_in = self._stage_midpoint(midpoint, total) if midpoint is not None else None
        # explicit idxs or injected draws may put a value goal at or before its
        # sample: such a call has the kernel count those samples and reads the
        # count back (one sync); Philox draws on the pick table cannot
        checked = idxs is not None or bool(draws) or mid_in is not None
        plain_call = not checked and crop_from is None and not record_draws
        hit = self._trl_cache.get(id(out)) if (out is not None and plain_call) else None
        if hit is not None and hit[0] is out and hit[1] == (B, nb):
            st = hit[2]
        else:
            st = self._trl_batch(total, record_draws, checked)
            if plain_call:
                self._remember(self._trl_cache, st[0], (B, nb), st)
        out, col_arr, ncols, outs, vcol_arr, nvcols, vidx, mcol_arr, nmcols, midx, idx_t, bad, _ = st
        dr, staged, rec, rec_t = self._stage(total, idxs, draws, record_draws)
        mid_rec = torch.empty(total, dtype=torch.int64, device=self.device) if record_draws else None
        seed, call = self._next_seed()
        stream = _lib.stream_of(self.device)
        L = self._L
        _lib.check(L.ogbx_trl_sample(self._buf, self._cfg, col_arr, ncols, B, nb, dr, _lib.ptr(mid_in), seed, call,
                                     outs, rec, _lib.ptr(mid_rec), stream), 'trl_sample')
        cf_out = None
        if self._visual:
            cf_out = torch.empty((total, 2), dtype=torch.int64, device=self.device) if (crop and record_draws) \
                else None
            F, draw = self._frame_stack or 1, int(crop and cf is None)
            _lib.check(L.ogbx_visual_gather(self._buf, None, vcol_arr, nvcols, total, vidx, F, CROP_PADDING,
                                            _lib.ptr(cf), draw, seed, call, _lib.ptr(cf_out), stream),
                       'visual_gather')
            # the crop draw is keyed by (sample, call) alone: the same offsets
            _lib.check(L.ogbx_visual_gather(self._buf, None, mcol_arr, nmcols, total, midx, F, CROP_PADDING,
                                            _lib.ptr(cf), draw, seed, call, None, stream), 'visual_gather')
        elif self._p_aug_live and not evaluation:
            np.random.rand()  # the coin; nothing of a non-visual batch is cropped
        del staged, cf, mid_in  # alive until the launches were issued
        if bad is not None:
            self._check_bad(bad, total, 'trl_sample')
        if record_draws:
            out.update(self._recorded(rec_t, idx_t, midpoint=mid_rec, crop_from=cf_out))
        return out

    def _sample_new(self, B, nb, idxs, draws, record_draws, keys, plain_call, shape):
        """A call into a new batch: allocate it, stage idxs / draws, launch
        through the plan (plain call; the batch's slot is remembered for
        ``out=``) or the direct entry point.  Returns the batch and the ``_*``
        keys a recording call adds to it."""
        torch = _torch()
        total = B * nb
        out, cols, scalars, keep, idx_t = self._batch(total, keys, record_draws)
        col_keep = (GcColumn * max(1, len(cols)))(*cols)
        col_arr = ctypes.cast(col_keep, ctypes.c_void_p)
        dr, staged, rec, rec_t = self._stage(total, idxs, draws, record_draws)
        seed, call = self._next_seed()
        stream = _lib.stream_of(self.device)
        if plain_call:
            plan = self._plan_for(seed)
            slot = self._next_slot()
            _lib.check(self._set_batch(plan, slot, col_arr, len(cols), B, nb, scalars), 'gc_plan_set_batch')
            # remember the batch's plan slot so that sample(..., out=this) skips
            # setup (the output tensors stay alive in `out` and `keep`)
            self._remember(self._out_cache, out, shape, slot, keep)
            st = self._L.ogbx_gc_plan_sample(plan, slot, call, stream)
        else:
            st = self._direct(col_arr, len(cols), B, nb, dr, seed, call, scalars, rec, stream)
        _lib.check(st, self._what)
        del staged, col_keep  # alive until the launch was issued
        if not record_draws or self._plain:
            return out, None
        return out, self._recorded(rec_t, idx_t)


# ----------------------------------------------------------------------------- HGCDataset


class HgcConfig(ctypes.Structure):
    _fields_ = [
        ('value_subgoal_steps', ctypes.c_int64),
        ('low_subgoal_steps', ctypes.c_int64),
        ('actor_subgoal_steps', ctypes.c_int64),
        ('has_low_value_goals', ctypes.c_int32),
        ('pad_', ctypes.c_int32),
        ('low_discount', ctypes.c_double),
        ('hv_mask_table', ctypes.c_void_p),
        ('hv_reward_table', ctypes.c_void_p),
        ('lv_mask_table', ctypes.c_void_p),
        ('lv_reward_table', ctypes.c_void_p),
    ]


class HgcDraws(ctypes.Structure):
    _fields_ = [('gc', GcDraws)] + [(k, ctypes.c_void_p) for k in _HDRAW_LOW]


class HgcDrawRecord(ctypes.Structure):
    _fields_ = [('gc', GcDrawRecord)] + [(k, ctypes.c_void_p) for k in _HDRAW_LOW]


_HGC_SCALARS = ('idxs', 'high_value_goal_idxs', 'high_actor_goal_idxs', 'low_value_goal_idxs',
                'high_value_offsets', 'high_value_subgoal_steps', 'high_value_masks', 'high_value_rewards',
                'low_value_subgoal_steps', 'low_value_masks', 'low_value_rewards', 'masks', 'rewards')


class HgcOutputs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in _HGC_SCALARS]


def _bind_hgc():
    L = _bind()
    if not getattr(L, '_hgc_bound', False):
        P = ctypes.POINTER
        L.ogbx_hgc_sample_ahead.restype = ctypes.c_int32
        L.ogbx_hgc_sample_ahead.argtypes = [
            P(GcBuffer), P(GcConfig), P(HgcConfig), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
            ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, P(HgcOutputs),
            ctypes.c_void_p,
        ]
        L.ogbx_hgc_sample.restype = ctypes.c_int32
        L.ogbx_hgc_sample.argtypes = [
            P(GcBuffer), P(GcConfig), P(HgcConfig), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
            ctypes.c_int64, P(HgcDraws), ctypes.c_uint64, ctypes.c_uint64, P(HgcOutputs), P(HgcDrawRecord),
            ctypes.c_void_p,
        ]
        L._hgc_bound = True
    return L


# What HGCDataset.sample returns after the dataset's own keys, in the reference's
# order (datasets.py:496-643): (key, source, select) is a gathered column, its
# source 'goal' being ``oracle_reps`` where the data has it and ``observations``
# otherwise (datasets.py:348-357); (key, 'scalar', dtype) a per-sample output of
# the kernel; (key, 'alias', other) the same tensor as ``other``.
_HGC_LAYOUT = (
    ('high_value_reps', 'alias', 'observations'),
    ('high_value_goals', 'goal', 2),
    ('high_value_actions', 'goal', 4),
    ('high_value_next_observations', 'observations', 4),
    ('high_value_offsets', 'scalar', 'int64'),
    ('high_value_subgoal_steps', 'scalar', 'int64'),
    ('high_value_masks', 'scalar', 'float64'),
    ('high_value_rewards', 'scalar', 'float64'),
    ('low_value_next_observations', 'observations', 5),
    ('low_value_subgoal_steps', 'scalar', 'int64'),
    ('low_value_masks', 'scalar', 'float64'),
    ('low_value_rewards', 'scalar', 'float64'),
    ('low_value_goals', 'goal', 6),  # with low_discount only
    ('value_goals', 'alias', 'high_value_goals'),
    ('masks', 'scalar', 'float64'),
    ('rewards', 'scalar', 'float64'),
    ('high_actor_goals', 'goal', 3),
    ('high_actor_actions', 'goal', 7),
    ('high_actor_next_observations', 'observations', 7),
    ('high_actor_targets', 'alias', 'high_actor_actions'),
    ('low_actor_goals', 'goal', 8),
    ('low_actor_goal_observations', 'observations', 8),
    ('low_actor_next_observations', 'observations', 9),
)


def _hgc_outputs(out, total, goal_src, has_low, device, own_reps=False):
    """Walk ``_HGC_LAYOUT`` over ``out``, which holds the data's own keys:
    aliases and scalar outputs are added here, and every gathered column is
    yielded as (key, src_key, select) for the caller to make ``out[key]``
    before the walk goes on.  own_reps: the caller has put
    ``high_value_reps``, the first key, there already (a visual batch, where it
    is no alias)."""
    torch = _torch()
    for key, what, arg in _HGC_LAYOUT[int(own_reps):]:
        if what == 'alias':
            out[key] = out[arg]
        elif what == 'scalar':
            out[key] = torch.empty(total, dtype=getattr(torch, arg), device=device)
        elif has_low or key != 'low_value_goals':
            yield key, (goal_src if what == 'goal' else what), arg


def _subgoal_tables(discount, K, gc_negative, device):
    """masks / rewards of HGCDataset.sample as functions of the clipped subgoal
    step count s in [0, K] (datasets.py:533-541, 550-556), computed with the
    reference's own float64 NumPy expressions so the device lookup is bit-exact."""
    torch = _torch()
    s = np.arange(K + 1, dtype=np.int64)
    succ = (s < K).astype(float)
    masks = 1.0 - succ
    rewards = -(1 - discount ** s) / (1 - discount) if gc_negative else (discount ** s) * succ
    return (torch.as_tensor(np.ascontiguousarray(masks), device=device),
            torch.as_tensor(np.ascontiguousarray(rewards, dtype=np.float64), device=device))


class _HgcHost:
    """What the hierarchical samplers (``HGCDataset``, ``HGCReplayBuffer``)
    put in place of ``_SamplerHost``'s hooks: the subgoal steps, tables and
    ``HgcConfig`` of a config, the image keys, the ``l_*`` draws and the walk
    that lays an HGC batch out."""

    _VISUAL_KEYS = ('observations', 'next_observations', 'high_value_reps', 'high_value_goals', 'high_value_actions',
                    'high_value_next_observations', 'low_value_next_observations', 'low_value_goals',
                    'high_actor_goals', 'high_actor_actions', 'high_actor_next_observations', 'low_actor_goals',
                    'low_actor_goal_observations', 'low_actor_next_observations')
    _CROP_KEYS = tuple(k for k in _VISUAL_KEYS if k not in ('high_value_reps', 'low_value_goals'))
    _TRL_OK = False

    def _init_hgc(self, config):
        """The subgoal steps as the reference resolves them
        (datasets.py:467-494), the mask / reward tables and ``_hcfg``."""
        c = config
        high = c.get('high_subgoal_steps', c['subgoal_steps'])
        self.value_subgoal_steps = int(high if c.get('value_subgoal_steps') is None else c['value_subgoal_steps'])
        self.actor_subgoal_steps = int(high if c.get('actor_subgoal_steps') is None else c['actor_subgoal_steps'])
        self.low_subgoal_steps = int(c.get('low_subgoal_steps', c['subgoal_steps']))
        self._has_low = c.get('low_discount') is not None
        self._draw_keys = _DRAW_ORDER + (_HDRAW_LOW if self._has_low else ())
        self._hv_tab = _subgoal_tables(c['discount'], self.value_subgoal_steps, c['gc_negative'], self.device)
        self._lv_tab = _subgoal_tables(c['discount'], self.low_subgoal_steps, c['gc_negative'], self.device)
        self._hcfg = HgcConfig(
            self.value_subgoal_steps, self.low_subgoal_steps, self.actor_subgoal_steps, int(self._has_low), 0,
            float(c['low_discount']) if self._has_low else 0.0,
            self._hv_tab[0].data_ptr(), self._hv_tab[1].data_ptr(),
            self._lv_tab[0].data_ptr(), self._lv_tab[1].data_ptr(),
        )

    def _hcfg_ptr(self):
        return ctypes.byref(self._hcfg)

    def _visual_indices(self, idx_t):
        return VisualIndices(*[idx_t['_' + k].data_ptr() for k in _HGC_SCALARS[:4]])

    def _draw_structs(self):
        dr = HgcDraws()
        return dr, dr.gc

    def _record_struct(self, rec_t):
        # the l_* draws exist (and are recorded) only with low_discount
        return HgcDrawRecord(super()._record_struct(rec_t), *[_lib.ptr(rec_t.get(k)) for k in _HDRAW_LOW])

    def _hgc_walk(self, total, record, vcols=None):
        """A new HGC batch: the data's own keys, then ``_HGC_LAYOUT``
        (``_hgc_outputs``).  Returns the batch in the reference's key order,
        the fused columns' descriptors (image columns go to ``vcols``),
        ``HgcOutputs`` and the index outputs of a recording call."""
        torch = _torch()
        out, cols = {}, []
        for src_key, key, select in self._own_columns():
            out[key] = self._gather(src_key, key, select, total, cols, vcols)
        if vcols is not None:
            # a visual batch's observations may be cropped; high_value_reps never is
            out['high_value_reps'] = self._gather('observations', 'high_value_reps', 0, total, cols, vcols)
        for key, src_key, select in _hgc_outputs(out, total, self._goal_source(), self._has_low, self.device,
                                                 own_reps=vcols is not None):
            out[key] = self._gather(src_key, key, select, total, cols, vcols)
        idx_t = {k: torch.empty(total, dtype=torch.int64, device=self.device)
                 for k in (_HGC_SCALARS[:4] if record else ())}
        outs = HgcOutputs(*[_lib.ptr(idx_t.get(k)) for k in _HGC_SCALARS[:4]],
                          *[out[k].data_ptr() for k in _HGC_SCALARS[4:]])
        return out, cols, outs, {'_' + k: t for k, t in idx_t.items()}


class HGCDataset(_HgcHost, GCDataset):
    """Hierarchical goal-conditioned sampler (reference: datasets.py:467-643).

    Extra config keys (as the reference): subgoal_steps, optional
    high_subgoal_steps, value_subgoal_steps, actor_subgoal_steps,
    low_subgoal_steps, low_discount.  One fused launch of hgc_sample_kernel
    per sample() returns the reference's 27 (28 with low_discount) keys.

    As a visual sampler (see GCDataset) it stacks every key the reference
    builds through get_observations / get_goal_observations / get_high_actions
    (the goal-type ones only without ``oracle_reps``) and crops exactly the
    keys of the reference's augment list (datasets.py:625-640):
    ``high_value_reps`` (bound to the observations before augment rebinds
    them) and ``low_value_goals`` (not in the list) stay uncropped.
    """

    def __init__(self, dataset, config, preprocess_frame_stack=True, seed=None):
        super().__init__(dataset, config, preprocess_frame_stack=preprocess_frame_stack, seed=seed)
        self._init_hgc(config)
        self._Lh = _bind_hgc()

    # sample() is GCDataset's; what differs for the hierarchical sampler
    # (with the hooks of _HgcHost):
    _what = 'hgc_sample'

    def _batch(self, total, keys, record, vcols=None):
        assert keys is None
        out, cols, outs, idx_t = self._hgc_walk(total, record, vcols)
        return out, cols, outs, (), idx_t

    def _set_batch(self, plan, slot, col_arr, ncols, B, nb, outs):
        return self._Lh.ogbx_gc_plan_set_batch(plan, slot, col_arr, ncols, B, nb, None, None, None, None, None,
                                               ctypes.byref(outs))

    def _direct(self, col_arr, ncols, B, nb, dr, seed, call, outs, rec, stream):
        return self._Lh.ogbx_hgc_sample(self._buf, self._cfg, self._hcfg, col_arr, ncols, B, nb, dr, seed, call,
                                        outs, rec, stream)


# ----------------------------------------------------------------------------- ATCDataset


class _AtcHost(_CallHost):
    """The host side that ``ATCDataset.sample`` and ``GCReplayBuffer.sample_atc``
    share: the batch layout and, in ``_atc_call``, every call that is not a
    steady ``out=`` refill (staging, the plain rule, the ``out=`` cache, the
    record tensors, the seed, the bad-sample readback, the ``_*`` keys).  The
    refill stays in line in both sample methods (``_CallHost._remember``): the
    ``k`` check, the family's staleness and empty tests, the coin, the lookup
    and on a hit the one ctypes call, so that it makes no Python call the
    written-out methods did not (profiles/atc_host_refactor_ab.txt).  A family
    supplies ``device``, ``_frame_stack``, ``_atc_cache``, ``_atc_source`` (its
    observations), ``_atc_launch`` (its entry point) and what follows."""

    _atc_out_strict = False  # an out= of another batch size raises ValueError (ATCDataset: builds a new batch)
    _atc_pick_checked = False  # an injected pick makes the call read its bad count back (the ring's empty valid(k))
    _atc_bad = None  # where an unchecked call counts its bad samples (the ring's device counter)
    _atc_bad_rows = None  # the family's message for bad explicit rows, over n, B and k

    def _atc_layout(self, src, B):
        """A new batch over the observations ``src``: the output dict (the
        reference's key order) and its column descriptor."""
        torch = _torch()
        shape = tuple(src.shape[1:])
        F = self._frame_stack or 1
        oshape = (B,) + shape[:-1] + (shape[-1] * F,) if shape else (B,)
        out = {k: torch.empty(oshape, dtype=src.dtype, device=self.device)
               for k in ('observations', 'positive_observations')}
        # an image is [H, W, C]; any other row is a 1-row image of its leading elements
        if len(shape) == 3:
            H, W = shape[0], shape[1]
        else:
            H, W = 1, int(np.prod(shape[:-1], dtype=np.int64))
        px = (shape[-1] if shape else 1) * src.element_size()
        col = AtcColumn(src.data_ptr(), out['observations'].data_ptr(), out['positive_observations'].data_ptr(),
                        H, W, px, int(src.dim() == 4))
        return out, col

    def _atc_call(self, B, k, crop, idxs, draws, record_draws, out, table):
        """Every call but the in-line refill: ``crop`` is the coin's answer,
        ``table`` what the family's ``_atc_launch`` takes first."""
        torch = _torch()
        draws = dict(draws or {})
        crop_from, pick = draws.pop('crop_from', None), draws.pop('pick', None)
        if draws:
            raise ValueError(f'unknown draw {sorted(draws)[0]!r}')
        cf = pk = ix = None
        if crop and crop_from is not None:
            cf = self._stage_crop_from(crop_from, B)
        if pick is not None:
            pk = self._stage_flat(pick, B, "draw 'pick'")
        if idxs is not None:
            ix = self._stage_flat(idxs, B, 'idxs')
        plain = ix is None and pk is None and crop_from is None and not record_draws
        hit = self._atc_cache.get(id(out)) if (out is not None and plain) else None
        fresh = hit is None or hit[0] is not out or hit[1] != B
        if not fresh:  # a refill whose draws held only None
            col = hit[2]
        else:
            if self._atc_out_strict and out is not None and len(out['observations']) != B:
                raise ValueError(f"out= holds a batch of {len(out['observations'])} samples, not {B}")
            out, col = self._atc_layout(self._atc_source(), B)
        rec = {}
        if record_draws:
            rec = dict(idxs=torch.empty(B, dtype=torch.int64, device=self.device),
                       pick=torch.empty(B, dtype=torch.int64, device=self.device))
            if crop:
                rec['crop_from'] = torch.empty((B, 2), dtype=torch.int64, device=self.device)
        # explicit rows (over the ring, injected picks too) are counted apart and the count
        # is read back (one sync); the Philox path counts into the family's counter, if any
        checked = ix is not None or (pk is not None and self._atc_pick_checked)
        bad = torch.zeros(1, dtype=torch.int64, device=self.device) if checked else self._atc_bad
        outs = AtcOutputs(_lib.ptr(rec.get('idxs')), _lib.ptr(rec.get('pick')), _lib.ptr(rec.get('crop_from')),
                          _lib.ptr(bad))
        if plain and fresh:
            self._remember(self._atc_cache, out, B, col, outs)  # what a refill passes on
        seed, call = self._next_seed()
        self._atc_launch(table, col, B, k, ix, pk, cf, int(crop and cf is None), seed, call, outs)
        del cf, pk  # alive until the launch was issued
        if checked:
            nbad = int(bad.item())
            if nbad and ix is not None:
                raise ValueError(self._atc_bad_rows.format(n=nbad, B=B, k=k))
            if nbad:
                raise ValueError(f'No valid ATC indices found for k={k}.')
        if record_draws:
            out['_idxs'] = rec.pop('idxs')
            out['_draws'] = rec
        return out


class ATCDataset(_AtcHost):
    """Anchor / positive observation pairs for ATC pretraining (reference:
    datasets.py:369-464; consumed by impls/pretrain_atc.py:167-251).

    config keys read (as the reference): frame_stack, p_aug, augment_padding
    (default 4).  ``sample(batch_size, k)`` returns ``observations`` (rows
    idx) and ``positive_observations`` (rows idx + k), idx drawn uniformly from
    valid(k): the candidates c (``dataset.valid_idxs`` when the dataset has
    'valids', else every row), in order, with c + k inside c's trajectory.
    ONE launch of ``atc_sample_kernel`` (``ogbx_atc_sample``,
    include/ogbx_atc.h) draws, stacks, crops and writes both keys.

    With ``frame_stack = F`` both keys hold F frames stacked on the last axis,
    channel block j the frame at row max(r - (F-1-j), first row of r's
    trajectory); this needs a compact dataset (no 'next_observations').
    ``preprocess_frame_stack`` is accepted and has no effect: the reference's
    two settings give identical batches, and here the frames always stay
    unstacked in HBM, so ``sampler.dataset['observations']`` stays unstacked.
    With ``p_aug > 0`` a call whose coin comes up (one ``np.random.rand()``
    per call, not under ``evaluation``; the rule of GCDataset) draws one
    offset pair per sample on the device and crops both keys with it when the
    observations are 4-D.

    valid(k).  On a periodic layout (``periodic_layout``: equal trajectories,
    the OGBench layout) a pick's row is a closed form of k and no table is
    built.  Otherwise valid(k) is compacted on the device
    (``ogbx_atc_valid_idxs``) once per k and kept in a cache of at most
    ``TABLE_CACHE`` tables, the least recently used dropped: a training run
    draws k from k_min..k_max on every step, and a table is 8 bytes per row.
    An empty valid(k) raises the reference's ValueError, decided on the host
    before any sample launch; k < 0 raises ValueError too (the reference would
    wrap around the buffer).

    ``draws`` takes ``'pick'`` (positions into valid(k)) and ``'crop_from'``
    ([B, 2], used when the call crops); ``record_draws`` adds ``_idxs`` and
    ``_draws`` (``pick``, and ``crop_from`` on a call whose coin came up).
    Explicit ``idxs`` that leave their trajectory (or the buffer) raise
    ValueError with their count, read back after the launch; the Philox path
    reads nothing back.  ``out=`` refills a batch returned by an earlier plain
    call with the same batch_size in place (stream ordered) and returns it; k
    may differ between the calls.  Seeds and calls are counted as in
    GCDataset.  ``sampler.dataset`` may be reassigned and its observations
    replaced or modified in place; the trajectory layout (fixed at
    construction, as the reference's ``__post_init__`` fixes its own) must
    stay.
    """

    TABLE_CACHE = 16  # valid(k) tables kept (non-periodic layouts)

    def __init__(self, dataset, config, preprocess_frame_stack=True, seed=None, _periodic=True):
        torch = _torch()
        if not isinstance(dataset, Dataset):
            dataset = Dataset(dataset)
        self.dataset = dataset
        self.config = config
        self.preprocess_frame_stack = preprocess_frame_stack
        self.size = dataset.size
        self.device = dataset.device
        fs = config.get('frame_stack')
        self._frame_stack = int(fs) if fs is not None else None
        if fs is not None:
            # only compact (observation-only) datasets (datasets.py:395-396)
            assert 'next_observations' not in dataset
            assert 1 <= self._frame_stack <= 8 and dataset['observations'].dim() >= 2
        self._padding = int(config.get('augment_padding', ATC_CROP_PADDING))
        if self._padding < 0:
            raise ValueError(f'augment_padding must be >= 0, got {self._padding}')
        self._p_aug = config.get('p_aug')
        self._p_aug_live = self._p_aug is not None and float(self._p_aug) > 0.0  # GCDataset's coin rule
        L = self._L = _bind()
        stream = _lib.stream_of(self.device)
        if 'terminals' in dataset:
            self.terminal_locs = nonzero_positive(dataset['terminals'])
        else:
            self.terminal_locs = torch.tensor([self.size - 1], dtype=torch.int64, device=self.device)
        assert self.terminal_locs.numel() > 0 and int(self.terminal_locs[-1]) == self.size - 1
        self.initial_locs = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device),
                                       self.terminal_locs[:-1] + 1])
        self.traj_end = torch.empty(self.size, dtype=torch.int64, device=self.device)
        _lib.check(L.ogbx_gc_traj_end(_lib.ptr(self.terminal_locs), self.terminal_locs.numel(), self.size,
                                      _lib.ptr(self.traj_end), stream))
        # the candidates (datasets.py:422-425)
        valid = dataset.valid_idxs if 'valids' in dataset else None
        self._cand = valid
        self.period = (0, 0, 0)
        if _periodic and (valid is None or valid.numel() > 0):
            self.period = periodic_layout(self.size, valid, self.traj_end[valid] if valid is not None
                                          else self.traj_end)
        self._buf = GcBuffer(self.size, _lib.ptr(valid), valid.numel() if valid is not None else 0,
                             self.traj_end.data_ptr(), None, None, *self.period)
        self._tables = {}  # k -> (valid(k) or None, its size), least recently used first
        self._seed = int(seed) if seed is not None else None
        self._calls = 0
        self._atc_cache = {}
        self._tok_ds, self._tok_gen = dataset, dataset._gen
        self._obs = dataset['observations']

    # ---------------------------------------------------------------- valid(k)
    def _valid_k(self, k):
        """(valid(k) as a device tensor, or None on a periodic layout; its size)."""
        P, pp, E = self.period
        if P > 0:
            return None, (self.size // P) * max(0, min(pp, E - k + 1))
        hit = self._tables.pop(k, None)
        if hit is None:
            torch = _torch()
            ncand = self._cand.numel() if self._cand is not None else self.size
            rows = torch.empty(max(ncand, 1), dtype=torch.int64, device=self.device)
            cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
            _lib.check(self._L.ogbx_atc_valid_idxs(self._buf, k, _lib.ptr(rows), _lib.ptr(cnt),
                                                   _lib.stream_of(self.device)), 'atc_valid_idxs')
            n = int(cnt.item())
            # a copy of its own size: the slice would keep all candidates' bytes alive
            hit = (rows[:n].clone() if n else None, n)
            while len(self._tables) >= max(1, self.TABLE_CACHE):
                del self._tables[next(iter(self._tables))]
        self._tables[k] = hit  # most recently used last
        return hit

    # ------------------------------------------------------------------ batches
    def _refresh(self):
        """The dataset object or one of its columns was replaced: the prepared
        batches hold the old observations' pointer."""
        ds = self.dataset
        if not isinstance(ds, Dataset):
            ds = self.dataset = Dataset(ds)
        obs = ds['observations']
        if obs.shape != self._obs.shape or obs.dtype != self._obs.dtype or obs.device != self._obs.device:
            raise ValueError("dataset column 'observations' changed shape, dtype or device after the sampler was "
                             'built')
        self._obs = obs
        self._atc_cache.clear()
        self._tok_ds, self._tok_gen = ds, ds._gen

    # ------------------------------------------------- what _AtcHost asks for
    _atc_bad_rows = ('atc_sample: {n} of {B} samples have idx + k (k={k}) past the end of their trajectory, or idx '
                     'outside the dataset')

    def _atc_source(self):
        return self._obs

    def _batch(self, B):
        """A new batch over the dataset's observations (tests build their column through it)."""
        return self._atc_layout(self._obs, B)

    def _atc_launch(self, valid, col, B, k, ix, pk, cf, draw, seed, call, outs):
        _lib.check(self._L.ogbx_atc_sample(
            self._buf, col, B, k, _lib.ptr(valid[0]), valid[1], self._frame_stack or 1, self._padding, _lib.ptr(ix),
            _lib.ptr(pk), _lib.ptr(cf), draw, seed, call, outs, _lib.stream_of(self.device)), 'atc_sample')

    def sample(self, batch_size, k, evaluation=False, idxs=None, draws=None, record_draws=False, out=None):
        """ATCDataset.sample (datasets.py:401-415), one launch.

        k: the temporal offset, an int >= 0.
        idxs: explicit anchor rows (each with idx + k inside its trajectory).
        draws: optional dict of injected reference draws: ``'pick'``, the
        positions into valid(k) of np.random.choice (datasets.py:404), and
        ``'crop_from'``, the [batch_size, 2] offsets of augment()'s randint
        (datasets.py:442), used when the call's coin comes up.
        record_draws: also return ``_idxs`` and the draws the kernel used
        (``_draws``).
        out: a batch returned by an earlier call with the same batch_size (and
        no idxs / draws / record_draws): refilled in place, stream ordered,
        and returned.
        """
        B, k = int(batch_size), operator.index(k)
        if k < 0:
            raise ValueError(f'k must be >= 0, got {k}')
        ds = self.dataset
        if ds is not self._tok_ds or getattr(ds, '_gen', None) != self._tok_gen:
            self._refresh()
        valid = self._valid_k(k)
        if valid[1] == 0:
            raise ValueError(f'No valid ATC indices found for k={k}.')
        # the coin stays on the host (datasets.py:411-412); the offsets are device draws
        crop = bool(self._p_aug_live and not evaluation and np.random.rand() < self._p_aug)
        # the conservative form of _atc_call's plain rule: a draws dict that holds only None goes there
        plain = idxs is None and not draws and not record_draws
        hit = self._atc_cache.get(id(out)) if (out is not None and plain) else None
        if hit is None or hit[0] is not out or hit[1] != B:
            return self._atc_call(B, k, crop, idxs, draws, record_draws, out, valid)
        seed, call = self._next_seed()
        _lib.check(self._L.ogbx_atc_sample(
            self._buf, hit[2], B, k, _lib.ptr(valid[0]), valid[1], self._frame_stack or 1, self._padding, None, None,
            None, int(crop), seed, call, hit[3], _lib.stream_of(self.device)), 'atc_sample')
        return out


def _replay_dtypes():
    torch = _torch()
    # ogbx_replay_dtype
    return {torch.bool: 0, torch.uint8: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}


class _BufferHost(_CallHost):
    """The host side that ``ReplayBuffer`` and the ring buffers share (each is
    also a ``Dataset`` of device columns): staging of what an insert takes, the
    cached insert descriptors, the descriptor of a gathered column and the
    ``out=`` cache (``_out_cache``, emptied when a column was replaced)."""

    def _init_host(self, seed):
        self._L = _bind()
        self._dtype_code = _replay_dtypes()
        self._seed = int(seed) if seed is not None else None
        self._calls = 0
        self._ins_cache = {}
        self._out_cache = {}
        self._out_gen = self._gen
        self._dev_idx = self.device.index
        torch = _torch()
        self._raw_stream = torch._C._cuda_getCurrentRawStream  # hipStream_t of the current stream, as an int
        self._new = torch.empty  # a new batch allocates a tensor per key

    def _source(self, key, v, n):
        """One leaf of an insert as a contiguous device tensor of n rows."""
        torch = _torch()
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(np.ascontiguousarray(v))
        if v.device != self.device:
            v = v.to(self.device)
        if v.dtype not in self._dtype_code:
            raise ValueError(f'{key!r}: unsupported source dtype {v.dtype}')
        col = self[key]
        if v.dim() == 0 or v.shape[0] != n or tuple(v.shape[1:]) != tuple(col.shape[1:]):
            raise ValueError(f'{key!r}: expected shape {(n,) + tuple(col.shape[1:])}, got {tuple(v.shape)}')
        return v if v.is_contiguous() else v.contiguous()

    def _mask(self, name, m, n):
        torch = _torch()
        if m is None:
            return None
        if not isinstance(m, torch.Tensor):
            m = torch.as_tensor(np.ascontiguousarray(m))
        if m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'{name} must be bool or uint8, got {m.dtype}')
        if m.device != self.device:
            m = m.to(self.device)
        if m.dim() != 1 or not m.is_contiguous():
            m = m.reshape(-1).contiguous()
        if m.shape[0] != n:
            raise ValueError(f'{name} must have {n} entries, got {m.shape[0]}')
        return m  # the kernel reads bytes; torch's bool bytes are 0 / 1

    def _check_keys(self, keys):
        if set(keys) != set(self.keys()):
            raise ValueError(f'the transition has keys {sorted(keys)}, the buffer {sorted(self.keys())}')

    def _column_of(self, key, rows):
        """The buffer's column ``key``, still the ``rows`` contiguous rows on
        the buffer's device that the kernels index."""
        col = self[key]
        if len(col) != rows or not col.is_contiguous() or col.device != self.device:
            raise ValueError(f'buffer column {key!r} was replaced by one of another length, layout or device')
        return col

    def _insert_columns(self, specs, rows, call_key, max_cols=None):
        """The ``ReplayInsertColumn`` array of an insert into columns of
        ``rows`` rows.  specs: (key, src, alt or None, op) per column, staged
        by ``_source``.  Cached under what the descriptors depend on: the
        sources' addresses and dtypes, the buffer's generation and
        ``call_key``, the call's other pointers."""
        key = call_key + (self._gen,) + tuple(
            (k, s.data_ptr(), s.dtype, a.data_ptr() if a is not None else 0, op) for k, s, a, op in specs)
        arr = self._ins_cache.get(key)
        if arr is None:
            code = self._dtype_code
            cols = []
            for k, s, a, op in specs:
                col = self._column_of(k, rows)
                if col.dtype not in code or col.dtype is _torch().bool:
                    raise ValueError(f'{k!r}: unsupported column dtype {col.dtype}')
                if a is not None and a.dtype != s.dtype:
                    raise ValueError(f'{k!r}: the alternative source has dtype {a.dtype}, the source {s.dtype}')
                row = col[0].numel() if col.dim() > 1 else 1
                cols.append(ReplayInsertColumn(col.data_ptr(), s.data_ptr(), a.data_ptr() if a is not None else None,
                                               row, code[s.dtype], code[col.dtype], op, 0))
            if max_cols is not None and len(cols) > max_cols:
                raise ValueError(f'at most {max_cols} columns per insert, got {len(cols)}')
            arr = (ReplayInsertColumn * len(cols))(*cols)
            if len(self._ins_cache) >= 8:
                self._ins_cache.clear()
            self._ins_cache[key] = arr
        return arr

    def _gather_column(self, src_key, B, select, rows):
        """(destination of B rows, descriptor) of one gathered column."""
        src = self[src_key]
        if len(src) != rows or not src.is_contiguous() or src.device != self.device:
            self._column_of(src_key, rows)  # raises: the column was replaced
        dst = self._new((B,) + tuple(src.shape[1:]), dtype=src.dtype, device=self.device)
        row_bytes = (src[0].numel() if src.dim() > 1 else 1) * src.element_size()
        return dst, GcColumn(src.data_ptr(), dst.data_ptr(), row_bytes, select, 0)


class ReplayBuffer(_BufferHost, Dataset):
    """Replay buffer on the device (reference: datasets.py:86-146; used by
    data_gen_scripts/main_sac.py:66-137): a ``Dataset`` whose rows are written
    by batched ring inserts and drawn uniformly from the rows held so far.

    ``create``, ``create_from_initial_dataset``, ``max_size``, ``size``,
    ``pointer``, ``add_transition`` and ``clear`` are the reference's.
    ``add_transitions`` / ``add_step`` insert one row per env in ONE launch of
    ``replay_insert_kernel``, ``sample`` / ``get_subset`` are ONE launch of
    ``replay_sample_kernel`` (include/ogbx_replay.h).

    The result of ``add_transitions`` is that of N sequential reference
    ``add_transition`` calls in row order: with M rows kept, the j-th kept row
    lands at ``(pointer + j) % max_size``, ``pointer' = (pointer + M) %
    max_size`` and ``size' = max(size, min(pointer + M, max_size - 1))``.  The
    last rule is the reference's quirk, kept on purpose: it computes ``size =
    max(pointer, size)`` after the modulo, so ``size`` stops at ``max_size -
    1`` and the buffer's last row is written but never drawn (a buffer of 5
    after 7 adds has pointer 2 and size 4).

    ``pointer`` and ``size`` live in a device-side header; no path of insert or
    sample reads it back.  The host mirrors both exactly while no insert had a
    ``keep`` mask; after a masked insert the ``pointer`` / ``size`` properties
    read the header back, which synchronises with the stream (and makes the
    mirror exact again).

    ``create_from_initial_dataset`` sets ``pointer = size = len(init)``.  When
    that equals ``max_size``, ``sample`` covers every row and the next add
    raises ``IndexError``, as the reference does (a masked add too, whatever
    its mask keeps: the host does not know the count).

    Values are cast to the column's dtype as a NumPy assignment casts them,
    for in-range values (sources bool, uint8, int32, int64, float32, float64;
    columns uint8, int32, int64, float32, float64).  A buffer with a 'valids'
    key is refused (the reference would draw from an empty ``valid_idxs``),
    as are columns of unequal length.

    ``sample`` draws with the plain sampler's Philox words: at one ``(seed,
    call)`` a buffer of size s returns, bit for bit, what ``Dataset({k: v[:s]})
    .sample`` returns.  An empty buffer raises ValueError when the host knows
    the size is 0; when it does not (a masked insert came last), every sample
    reads row 0 and the kernel adds the batch size to a device counter, read by
    ``empty_draws()``.
    """

    SAC_KEYS = ('observations', 'actions', 'rewards', 'masks', 'next_observations')  # main_sac.py:115-123

    @classmethod
    def create(cls, transition, size, device=None, seed=None):
        """Zero buffers ``[size, *shape]`` with the dtype of
        ``np.array(example)`` (datasets.py:92-106): ``rewards=0.0`` gives a
        float64 column."""
        torch = _torch()
        if device is None:
            device = 'cuda'
        size = operator.index(size)
        if size <= 0:
            raise ValueError(f'size must be > 0, got {size}')
        cols = {}
        for k, example in transition.items():
            if isinstance(example, torch.Tensor):
                shape, dtype = tuple(example.shape), example.dtype
            else:
                example = np.array(example)
                shape, dtype = example.shape, torch.from_numpy(np.zeros(0, example.dtype)).dtype
            cols[k] = torch.zeros((size,) + tuple(shape), dtype=dtype, device=device)
        return cls(cols, device=device, seed=seed)

    @classmethod
    def create_from_initial_dataset(cls, init_dataset, size, device=None, seed=None):
        """Buffers of ``size`` rows holding ``init_dataset`` in front, with
        ``pointer = size = len(init_dataset)`` (datasets.py:108-125)."""
        torch = _torch()
        size = operator.index(size)
        if device is None:
            device = getattr(init_dataset, 'device', 'cuda')
        init = {k: _to_device(v, device) for k, v in init_dataset.items()}
        n = max(len(v) for v in init.values())
        if size <= 0 or n > size:
            raise ValueError(f'the initial dataset has {n} rows, the buffer {size}')
        cols = {}
        for k, v in init.items():
            cols[k] = torch.zeros((size,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device)
            cols[k][: len(v)] = v
        rb = cls(cols, device=device, seed=seed)
        rb._set_header(n, n)
        return rb

    def __init__(self, data=(), device=None, seed=None, **kw):
        torch = _torch()
        data = dict(data, **kw)
        if 'valids' in data:
            raise ValueError("a ReplayBuffer cannot have a 'valids' column (the reference would draw from an "
                             'empty valid_idxs)')
        self._hdr = None
        super().__init__(data, device=device)
        lens = {len(v) for v in self.values()}
        if len(lens) != 1:
            raise ValueError(f'every column of a ReplayBuffer needs the same number of rows, got {sorted(lens)}')
        self.max_size = lens.pop()
        self._init_host(seed)
        self._hdr = torch.zeros(4, dtype=torch.int64, device=self.device)  # OGBX_REPLAY_HEADER_WORDS
        self._empty = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._parity = 0
        self._h_pointer = self._h_size = 0
        self._known = True

    # ------------------------------------------------------------------ header
    def _set_header(self, pointer, size):
        torch = _torch()
        pointer, size = operator.index(pointer), operator.index(size)
        if not (0 <= pointer <= self.max_size and 0 <= size <= self.max_size):
            raise ValueError(f'pointer and size must lie in [0, {self.max_size}]')
        row = torch.tensor([pointer, size, pointer, size], dtype=torch.int64)
        self._hdr.copy_(row.to(self.device))
        self._h_pointer, self._h_size, self._known = pointer, size, True

    def _read_header(self):
        if not self._known:
            h = self._hdr.cpu()  # synchronises with the stream
            self._h_pointer, self._h_size = int(h[2 * self._parity]), int(h[2 * self._parity + 1])
            self._known = True

    @property
    def size(self):
        self._read_header()
        return self._h_size

    @size.setter
    def size(self, value):
        if self._hdr is None:  # Dataset.__init__'s row count: max_size
            return
        self._read_header()
        self._set_header(self._h_pointer, value)

    @property
    def pointer(self):
        self._read_header()
        return self._h_pointer

    @pointer.setter
    def pointer(self, value):
        self._read_header()
        self._set_header(value, self._h_size)

    def clear(self):
        """size = pointer = 0, on the stream (datasets.py:144-146); the rows
        stay where they are."""
        _lib.check(self._L.ogbx_replay_clear(_lib.ptr(self._hdr), _lib.stream_of(self.device)), 'replay_clear')
        self._h_pointer = self._h_size = 0
        self._known = True

    def empty_draws(self):
        """Samples drawn so far while the buffer was empty and the host did not
        know it (each read row 0).  Reads the device counter: synchronises."""
        return int(self._empty.item())

    # ------------------------------------------------------------------ inserts
    def _insert(self, specs, n, keep, alt_select):
        """specs: (key, src, alt or None, op) per column, already staged by
        ``_source``.  One launch; the host mirror follows when no mask."""
        if n > self.max_size:
            raise ValueError(f'{n} rows in one insert exceed max_size {self.max_size} (two rows would race for one '
                             'slot)')
        if n == 0:
            return
        if self._known and self._h_pointer >= self.max_size:
            raise IndexError(f'index {self._h_pointer} is out of bounds for axis 0 with size {self.max_size}')
        arr = self._insert_columns(
            specs, self.max_size,
            (n, keep.data_ptr() if keep is not None else 0, alt_select.data_ptr() if alt_select is not None else 0),
            max_cols=REPLAY_MAX_COLS)
        st = self._L.ogbx_replay_insert(self._hdr.data_ptr(), self._parity, self.max_size, arr, len(arr), n,
                                        _lib.ptr(keep), _lib.ptr(alt_select), self._raw_stream(self._dev_idx))
        if st:
            _lib.check(st, 'replay_insert')
        self._parity ^= 1
        if keep is not None:
            self._known = False
        elif self._known:
            self._h_pointer, self._h_size = self._after(self._h_pointer, self._h_size, n, self.max_size)

    @staticmethod
    def _after(pointer, size, m, max_size):
        """(pointer, size) after m >= 1 sequential reference adds: size' is the
        largest pointer value visited, max(size, min(pointer + m, max_size - 1))
        in every state the buffer reaches by itself (size >= pointer)."""
        end = pointer + m
        top = end if end < max_size else (max_size - 1 if pointer < max_size - 1 else m - 1)
        return end % max_size, max(size, top)

    def add_transitions(self, batch, keep=None):
        """Insert one row per env: every leaf of ``batch`` has a leading N.
        ``keep`` (bool / uint8 ``[N]``): only the kept rows are added, in row
        order.  N > max_size and keys that differ from the buffer's raise
        ValueError."""
        self._check_keys(batch)
        first = next(iter(batch.values()))
        n = len(first)
        specs = [(k, self._source(k, batch[k], n), None, REPLAY_OP_NONE) for k in self]
        self._insert(specs, n, self._mask('keep', keep, n), None)

    def add_transition(self, transition):
        """One transition whose leaves have no batch axis (datasets.py:134-142)."""
        torch = _torch()
        self._check_keys(transition)
        batch = {}
        for k, v in transition.items():
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            batch[k] = v.reshape((1,) + tuple(self[k].shape[1:]))
        self.add_transitions(batch)

    def add_step(self, observations, actions, rewards, terminated, next_observations, final_observation=None,
                 done=None, keep=None):
        """Insert what a vectorized env's ``step`` returned as the reference's
        SAC transitions (main_sac.py:115-123) in one launch:
        ``masks = 1 - terminated`` and ``next_observations`` taken from
        ``final_observation`` (``info['final_observation']`` of an
        ``auto_reset=True`` env) where ``done`` (bool / uint8 ``[N]``,
        terminated | truncated) is set.  The buffer's keys must be
        ``SAC_KEYS``.

        ``observations`` must be a tensor the caller still owns: the env's
        observation view is overwritten by the step that produced
        ``next_observations``, so pass a copy taken before that step."""
        self._check_keys(self.SAC_KEYS)
        if (final_observation is None) != (done is None):
            raise ValueError('final_observation and done go together')
        n = len(observations)
        src = dict(observations=observations, actions=actions, rewards=rewards, masks=terminated,
                   next_observations=next_observations)
        alt = self._source('next_observations', final_observation, n) if final_observation is not None else None
        specs = []
        for k in self:
            specs.append((k, self._source(k, src[k], n), alt if k == 'next_observations' else None,
                          REPLAY_OP_ONE_MINUS if k == 'masks' else REPLAY_OP_NONE))
        self._insert(specs, n, self._mask('keep', keep, n), self._mask('done', done, n))

    # ----------------------------------------------------------------- sampling
    def _batch(self, B, record_idxs):
        torch = _torch()
        out, cols = {}, []

        gather, rows = self._gather_column, self.max_size
        for k in self.keys():
            out[k], col = gather(k, B, 0, rows)
            cols.append(col)
        if 'next_observations' not in self:
            out['next_observations'], col = gather('observations', B, 1, rows)  # datasets.py:81-82
            cols.append(col)
        if len(cols) > REPLAY_MAX_COLS:
            raise ValueError(f'at most {REPLAY_MAX_COLS} columns per sample, got {len(cols)}')
        idx = torch.empty(B, dtype=torch.int64, device=self.device) if record_idxs else None
        if record_idxs:
            out['_idxs'] = idx
        return out, (GcColumn * len(cols))(*cols), len(cols), idx

    def sample(self, batch_size, idxs=None, out=None, record_idxs=False):
        """Dataset.sample (datasets.py:72-83) over rows ``[0, size)``, one
        launch: every column at the drawn (or given) rows, in the buffer's key
        order; without a ``next_observations`` column,
        ``next_observations = observations[min(idx + 1, size - 1)]`` with the
        CURRENT size.  Explicit ``idxs`` are clamped into ``[0, max_size)``.

        out: a batch returned by an earlier call with the same batch_size and
        record_idxs (and no idxs): refilled in place, stream ordered, and
        returned.
        record_idxs: also return the rows used (``out['_idxs']``).
        """
        torch = _torch()
        B = int(batch_size)
        ix = None
        if idxs is not None:
            ix = _to_device(idxs, self.device).to(torch.int64).reshape(-1)
            if ix.numel() != B:
                raise ValueError(f'idxs must have {B} entries, got {ix.numel()}')
        elif self._known and self._h_size == 0:
            raise ValueError('cannot sample from an empty ReplayBuffer')
        if self._out_gen != self._gen:  # a column was replaced
            self._out_cache.clear()
            self._out_gen = self._gen
        hit = self._out_cache.get(id(out)) if (out is not None and ix is None) else None
        if hit is not None and hit[0] is out and hit[1] == (B, record_idxs):
            arr, ncols, idx_out = hit[2]
        else:
            out, arr, ncols, idx_out = self._batch(B, record_idxs)
            if ix is None:
                self._remember(self._out_cache, out, (B, record_idxs), (arr, ncols, idx_out))
        seed, call = self._next_seed()
        st = self._L.ogbx_replay_sample(self._hdr.data_ptr(), self._parity, self.max_size, arr, ncols, B,
                                        _lib.ptr(ix), seed, call, _lib.ptr(idx_out), self._empty.data_ptr(),
                                        self._raw_stream(self._dev_idx))
        if st:
            _lib.check(st, 'replay_sample')
        return out

    def get_subset(self, idxs):
        return self.sample(len(idxs), idxs=idxs)

    def get_random_idxs(self, num_idxs):
        """Uniform rows of ``[0, size)`` (datasets.py:65-70)."""
        return self.sample(num_idxs, record_idxs=True)['_idxs']


class GCReplayBuffer(_SamplerHost, _AtcHost, _BufferHost, Dataset):
    """Hindsight goal sampling over an on-device episode ring: what batched
    envs produce, one row per env and step, sampled as the reference's
    ``GCDataset.sample`` (datasets.py:213-327) samples a dataset
    (include/ogbx_online.h).

    Layout.  ``num_envs = N`` lanes and ``horizon = T`` time slots; every
    insert takes exactly one row from every env, and the row of env e at
    logical step t lives at physical row ``(t % T) * N + e`` of every column
    (``[T * N, *shape]``).  The host counts the steps ``S`` (``steps``);
    ``L = min(S, T)`` of them are live (``live_steps``), ``S - L .. S - 1``.
    ``done[e]`` (terminated | truncated of an auto-reset env) closes env e's
    episode at that step.

    The snapshot (``snapshot()``) is the dataset of the live rows unrolled
    env-major -- flat index ``u = e * L + k`` holds env e at step
    ``S - L + k`` -- with ``terminals = 1`` on the last row of every closed
    episode and on every env's newest row (an open episode ends "now").  An
    episode whose head was overwritten starts at its oldest live row.
    ``sample`` returns, bit for bit, what ``GCDataset(Dataset(snapshot),
    config).sample`` returns under the same draws, for every key of the
    buffer, ``value_goals`` / ``actor_goals`` (from ``oracle_reps`` when the
    buffer has that column, else ``observations``), ``masks`` and ``rewards``;
    with the Philox draws at one ``(seed, call)`` too.  Every index it takes or
    reports (``idxs``, the draws' picks, ``_idxs`` and the goal indices of a
    recording call) is a flat index of the snapshot.  A ``terminals`` column of
    the buffer holds what was inserted (``add_step``: done); the snapshot's
    ``terminals`` also marks the newest rows.

    ``add`` / ``add_step`` are ONE launch of ``online_insert_kernel``, which
    also keeps the episode tables at O(1) per row (``ep_seq``, ``cur_seq``,
    ``ep_end``); ``sample`` is ONE launch of ``online_gc_sample_kernel``.
    Nothing is read back.  The regular layout only: the buffer stores its own
    ``next_observations``; no ``valids``.

    Visual buffers.  The config's ``frame_stack`` and ``p_aug`` are read by
    ``GCDataset``'s rules.  The ring and ``snapshot()`` always hold UNSTACKED
    frames (a ring of stacked frames would take F times the memory and insert
    traffic).  With ``frame_stack = F`` (1..8), ``observations`` and, without
    ``oracle_reps``, ``value_goals`` / ``actor_goals`` hold F frames joined on
    the last axis: channel block j of a selector row at step t of env e is the
    ``observations`` frame at step max(t - (F-1-j), s0), s0 the earliest step
    among t - (F-1) .. t that is live and of t's episode -- the reference's
    ``get_stacked_observations`` (datasets.py:359-366) over the snapshot, where
    an episode whose head was overwritten starts at its oldest live row.
    ``next_observations`` is the stack shifted by one: blocks 1 .. F-1 of the
    stacked ``observations`` followed by the buffer's own ``next_observations``
    row, which on every ``add_step`` history
    (``next_observations[t] == observations[t+1]`` inside an episode) is the
    reference's ``get_observations(idxs + 1)`` over the compact unrolling of
    the snapshot.  2-D observations stack to ``[B, F * D]``.  With
    ``p_aug > 0``, a call whose coin comes up (one ``np.random.rand()`` per
    call; none under ``evaluation=True`` or with ``p_aug`` None or <= 0) crops
    every 4-D key of ``_CROP_KEYS`` after stacking, with padding 3 and one
    ``(cy, cx)`` per sample, injected as ``draws['crop_from']`` (``[B, 2]``) or
    drawn on the device under the sampler's key at the call's
    ``(seed, call)`` (Philox slot ``OGBX_VISUAL_CROP_SLOT``; a recording call
    that cropped reports them as ``_draws['crop_from']``).  Such a ``sample``
    is TWO launches: the sample kernel over the non-image columns, then
    ``online_visual_gather_kernel`` (``ogbx_online_visual_gather``,
    include/ogbx_online_visual.h) over the image columns.  Indices, ``masks``,
    ``rewards`` and every non-image key are those of the same buffer without
    the two keys at the same seed and call, which still issues the one launch.

    TRL buffers.  With ``config['agent_name']`` in ``TRL_AGENTS`` ``sample``
    runs the reference's TRL branch (datasets.py:198-204, 254-276) over the
    snapshot: ``idxs`` and the random goals come only from the rows that are
    not the last of their trajectory -- every live row but the last row of
    each closed episode and each env's newest row -- and the batch carries the
    value-midpoint keys in the reference's order, with ``GCDataset``'s rule of
    one tensor per distinct (source, selector): ``actor_goal_observations is
    value_goal_observations``; without ``oracle_reps`` also
    ``value_goal_observations is value_goals``, ``value_midpoint_goals is
    value_midpoint_observations`` and ``value_cur_goals is observations``; with
    it ``value_cur_goals is oracle_reps``.  ``value_next_goals`` and
    ``next_actions`` gather at flat row min(u + 1, L * N - 1), the snapshot's
    ``observations[idxs + 1]`` / ``actions[idxs + 1]`` -- not the buffer's own
    ``next_observations`` column, which differs from it at an auto-reset.
    ``value_offsets`` / ``value_midpoint_offsets`` are int64.  The buffer
    needs an ``actions`` column and ``steps >= 2`` to sample.

    That pick table changes with every insert and is never built.  The buffer
    keeps ``P``, the exclusive prefix sum over envs of their pickable rows
    (``L - 1`` minus the episodes the env closed before its newest row, from
    two rows of ``ep_seq``), and rebuilds it inside ``sample`` -- one scan,
    ``ogbx_online_trl_table`` -- when ``steps``, the count of ``clear()``
    calls or the stream changed since the last build (``trl_table_builds``
    counts the builds): a sample after an insert is the scan and one launch of
    ``online_trl_sample_kernel``, further samples at that step the one launch;
    ``add`` / ``add_step`` are untouched.  The kernel turns a pick into a row
    by a search over ``P`` for the env and one over the env's live closed
    episodes in ``ep_end`` (include/ogbx_online_trl.h).  ``draws`` takes
    ``'midpoint'`` and its ``pick`` / ``a_pick`` index the pick table;
    ``record_draws`` reports ``_value_midpoint_idxs``.  Calls with explicit
    ``idxs`` or injected draws read back the count of samples whose value goal
    is not past the sample and raise ValueError with it; the Philox path
    reads nothing back, and ``trl_bad_samples()`` reads its device counter,
    nonzero only when a call found every live row ending an episode.  The
    config needs ``value_p_curgoal == 0`` and ``value_p_randomgoal == 0``
    (ValueError, as ``GCDataset``); a TRL buffer with ``frame_stack`` or a
    live ``p_aug`` and ``HGCReplayBuffer`` with a TRL agent name raise
    NotImplementedError at construction.  A buffer without a TRL agent name
    keeps its ``sample``, its single launch and its batches.

    ATC pairs.  ``sample_atc(batch_size, k)`` returns what the reference's
    ``ATCDataset.sample(batch_size, k)`` (datasets.py:401-464) returns over
    the snapshot without its ``next_observations``: ``observations`` at
    anchors drawn from valid(k) -- every live row whose offset + k stays
    inside its episode -- and ``positive_observations`` k steps later, both
    stacked and cropped from the ring's ``observations`` column by the
    config's ``frame_stack`` / ``p_aug`` / ``augment_padding``.  valid(k) is
    never built: an episode shorter than k + 1 holds no anchor, so the count
    per env is a sum over its live episodes, which ``ogbx_online_atc_table``
    walks once per ``(steps, clears, stream, k)``; the sample's one launch
    turns a pick into a row by a search over the envs' prefix sum and one over
    the env's episodes (include/ogbx_online_atc.h).  Its tables are allocated
    by the first call: a buffer that never draws pairs holds none, and its
    ``sample`` is untouched.  Every buffer class and config takes it.
    """

    RESERVED = ('masks', 'rewards', 'value_goals', 'actor_goals', 'valids')
    STEP_KEYS = ('observations', 'actions', 'next_observations', 'terminals')
    # _SamplerHost reads the columns through ``dataset``: for a ring, the buffer itself
    dataset = property(lambda self: self)
    _VisualColumn = OnlineVisualColumn  # ogbx_online_visual_gather's descriptor

    @classmethod
    def create(cls, transition, num_envs, horizon, config, device=None, seed=None):
        """Zero columns ``[horizon * num_envs, *shape]`` with the dtype of
        ``np.array(example)``, as ``ReplayBuffer.create``."""
        torch = _torch()
        if device is None:
            device = 'cuda'
        num_envs, horizon = operator.index(num_envs), operator.index(horizon)
        if num_envs <= 0 or horizon <= 0:
            raise ValueError(f'num_envs and horizon must be > 0, got {num_envs} and {horizon}')
        cols = {}
        for k, example in transition.items():
            if isinstance(example, torch.Tensor):
                shape, dtype = tuple(example.shape), example.dtype
            else:
                example = np.array(example)
                shape, dtype = example.shape, torch.from_numpy(np.zeros(0, example.dtype)).dtype
            cols[k] = torch.zeros((horizon * num_envs,) + tuple(shape), dtype=dtype, device=device)
        return cls(cols, num_envs, horizon, config, device=device, seed=seed)

    def __init__(self, data, num_envs, horizon, config, device=None, seed=None):
        torch = _torch()
        data = dict(data)
        bad = [k for k in data if k in self.RESERVED]
        if bad:
            raise ValueError(f'a GCReplayBuffer cannot have columns named {bad}: sample() returns keys of these names')
        if 'observations' not in data:
            raise ValueError("a GCReplayBuffer needs an 'observations' column")
        self._steps = None
        super().__init__(data, device=device)
        self.num_envs, self.horizon = operator.index(num_envs), operator.index(horizon)
        if self.num_envs <= 0 or self.horizon <= 0:
            raise ValueError(f'num_envs and horizon must be > 0, got {num_envs} and {horizon}')
        self.rows = self.num_envs * self.horizon
        if {len(v) for v in self.values()} != {self.rows}:
            raise ValueError(f'every column of a GCReplayBuffer needs horizon * num_envs = {self.rows} rows')
        if len(self) + 2 > REPLAY_MAX_COLS:
            raise ValueError(f'at most {REPLAY_MAX_COLS - 2} columns (a batch adds the two goal columns)')
        self.config = config
        assert np.isclose(config['value_p_curgoal'] + config['value_p_trajgoal'] + config['value_p_randomgoal'], 1.0)
        assert np.isclose(config['actor_p_curgoal'] + config['actor_p_trajgoal'] + config['actor_p_randomgoal'], 1.0)
        self._cfg = _gc_config(config)
        self._init_host(seed)
        self._sample_entry = self._L.ogbx_online_gc_sample
        self.ep_seq = torch.zeros(self.horizon, self.num_envs, dtype=torch.int32, device=self.device)
        self.cur_seq = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.ep_end = torch.zeros(self.horizon, self.num_envs, dtype=torch.int64, device=self.device)
        self._ring = OnlineRing(self.num_envs, self.horizon, 0, self.ep_seq.data_ptr(), self.cur_seq.data_ptr(),
                                self.ep_end.data_ptr())
        self._done = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)  # add_step's terminated | truncated
        self._steps = 0
        self._clears = 0  # clear() calls: with ``steps``, what a table derived from the ring depends on
        self._frame_stack, self._p_aug, self._p_aug_live, self._visual = _visual_config(config, self)
        self._trl = config.get('agent_name') in TRL_AGENTS
        if self._trl:
            self._init_trl()  # binds sample on the instance too, for the same reason as below
        elif self._frame_stack is not None or self._p_aug_live:
            # bound here, on the instance, and not tested for inside sample():
            # a buffer without the two keys keeps its sample() as it was, the
            # steady refill's one lookup and one ctypes call (as GCDataset
            # binds its TRL sample)
            self.sample = self._sample_visual
            self._Lv = _online_visual.bind()
            self._vis_cache = {}

    # ------------------------------------------------------------------- state
    @property
    def steps(self):
        """S: the steps inserted since creation or ``clear()``."""
        return self._steps

    @property
    def live_steps(self):
        """L = min(S, T)."""
        return min(self._steps, self.horizon)

    @property
    def size(self):
        """Rows of the snapshot, L * N."""
        return self.live_steps * self.num_envs

    @size.setter
    def size(self, value):  # Dataset.__init__'s row count
        pass

    def clear(self):
        """S = 0 and every env's episode ordinal back to 0, on the stream; the
        rows stay where they are."""
        _lib.check(self._L.ogbx_online_clear(self._ring, _lib.stream_of(self.device)), 'online_clear')
        self._steps = self._ring.steps = 0
        self._clears += 1

    # ------------------------------------------------------------------ inserts
    def _insert(self, specs, done, alt_select):
        """specs: (key, src, alt or None, op) per column, staged by
        ``_source``.  One launch; then S + 1."""
        # (the constructor bounds the column count)
        arr = self._insert_columns(
            specs, self.rows, (done.data_ptr(), alt_select.data_ptr() if alt_select is not None else 0))
        st = self._L.ogbx_online_insert(self._ring, arr, len(arr), done.data_ptr(),
                                        alt_select.data_ptr() if alt_select is not None else None,
                                        self._raw_stream(self._dev_idx))
        if st:
            _lib.check(st, 'online_insert')
        self._steps += 1
        self._ring.steps = self._steps

    def add(self, batch, done):
        """Insert one step: every leaf of ``batch`` has a leading N and
        ``done`` is bool / uint8 ``[N]``.  A wrong N, keys that differ from the
        buffer's or a leaf of another shape raise ValueError."""
        self._check_keys(batch)
        n = self.num_envs
        specs = [(k, self._source(k, batch[k], n), None, REPLAY_OP_NONE) for k in self]
        self._insert(specs, self._mask('done', done, n), None)

    def add_step(self, observations, actions, terminated, truncated, next_observations, final_observation=None):
        """Insert what a vectorized env's ``step`` returned in one launch:
        ``observations``, ``actions``, ``next_observations`` -- taken from
        ``final_observation`` (``info['final_observation']`` of an
        ``auto_reset=True`` env) where done = terminated | truncated -- and
        ``terminals`` = done as float32.  The buffer's keys must be
        ``STEP_KEYS``.  ``truncated=None`` takes ``terminated`` as done;
        otherwise the two masks are combined by one elementwise op before the
        launch.

        ``observations`` must be a tensor the caller still owns: the env's
        observation view is overwritten by the step that produced
        ``next_observations``, so pass a copy taken before that step."""
        torch = _torch()
        self._check_keys(self.STEP_KEYS)
        n = self.num_envs
        done = self._mask('terminated', terminated, n)
        if truncated is not None:
            done = torch.logical_or(done, self._mask('truncated', truncated, n), out=self._done)
        src = dict(observations=observations, actions=actions, next_observations=next_observations, terminals=done)
        alt = self._source('next_observations', final_observation, n) if final_observation is not None else None
        specs = [(k, self._source(k, src[k], n), alt if k == 'next_observations' else None, REPLAY_OP_NONE)
                 for k in self]
        self._insert(specs, done, done if alt is not None else None)

    # ----------------------------------------------------------------- sampling
    def _gather(self, src_key, dst_key, select, B, cols, vcols):
        """The destination of one output column.  Its descriptor goes to
        ``vcols`` when it is an image column of a visual buffer, else to
        ``cols`` (the sample kernel's).  A stacked ``next_observations`` is the
        stack over ``observations`` with the buffer's own row as its newest
        block (``alt``)."""
        spec = self._visual_spec(src_key, dst_key) if vcols is not None else None
        if spec is None:
            dst, col = self._gather_column(src_key, B, select, self.rows)
            cols.append(col)
            return dst
        alt = None
        if dst_key == 'next_observations' and src_key == 'next_observations' and spec[0]:
            alt, src_key = self._column_of('next_observations', self.rows), 'observations'
        src = self._column_of(src_key, self.rows)
        if alt is not None and (alt.shape != src.shape or alt.dtype != src.dtype):
            raise ValueError("frame_stack needs 'next_observations' of the shape and dtype of 'observations'")
        dst, vc = self._image_column(src, (src.data_ptr(), alt.data_ptr() if alt is not None else None), select, spec,
                                     B)
        vcols.append(vc)
        return dst

    def _batch(self, B, record, vcols=None):
        torch = _torch()
        out, cols = self._gc_walk(B, vcols)
        if len(cols) > REPLAY_MAX_COLS:
            raise ValueError(f'at most {REPLAY_MAX_COLS} columns per sample, got {len(cols)}')
        out['masks'] = torch.empty(B, dtype=torch.float64, device=self.device)
        out['rewards'] = torch.empty(B, dtype=torch.float64, device=self.device)
        idx_t = {}
        if record:
            idx_t = {k: torch.empty(B, dtype=torch.int64, device=self.device)
                     for k in ('_idxs', '_value_goal_idxs', '_actor_goal_idxs')}
        arr = (GcColumn * len(cols))(*cols)
        batch = OnlineBatch(ctypes.cast(arr, ctypes.c_void_p), len(cols), 0, B,
                            *[t.data_ptr() for t in idx_t.values()] if record else (None, None, None),
                            out['masks'].data_ptr(), out['rewards'].data_ptr())
        return out, (batch, arr), idx_t

    def sample(self, batch_size, idxs=None, draws=None, record_draws=False, out=None, evaluation=False):
        """GCDataset.sample (datasets.py:213-294) over the snapshot, one
        launch.  Raises ValueError while no step was inserted.

        idxs: explicit flat rows of the snapshot, clamped into ``[0, L * N)``.
        draws: injected reference draws (``_DRAW_ORDER``), picks as flat rows;
        with ``p_aug`` also ``'crop_from'``, the ``[batch_size, 2]`` offsets
        (cy, cx) of augment()'s randint (datasets.py:333), used when the call
        crops.
        record_draws: also return the draws used (``out['_draws']``, with
        ``'crop_from'`` on a call that cropped) and the flat ``_idxs`` /
        ``_value_goal_idxs`` / ``_actor_goal_idxs``.
        out: a batch returned by an earlier plain call with the same
        batch_size: refilled in place, stream ordered, and returned (a batch
        of another size raises ValueError).
        evaluation: no augmentation and no coin (datasets.py:278); read only
        with ``frame_stack`` / ``p_aug`` (``_sample_visual``, which a buffer
        with either key runs in place of this method).

        ``HGCReplayBuffer.sample`` is this method over its own hooks:
        HGCDataset.sample (datasets.py:496-643) over the snapshot, one launch.
        With ``low_discount`` it also takes and records the ``l_*`` draws, and
        a recording call returns the flat ``_idxs`` /
        ``_high_value_goal_idxs`` / ``_high_actor_goal_idxs`` /
        ``_low_value_goal_idxs``.
        """
        B = int(batch_size)
        if self._steps == 0:
            raise ValueError(f'cannot sample from an empty {self._NAME}')
        plain = idxs is None and not draws and not record_draws
        if self._out_gen != self._gen:  # a column was replaced
            self._out_cache.clear()
            self._out_gen = self._gen
        hit = self._out_cache.get(id(out)) if (out is not None and plain) else None
        if hit is not None and hit[0] is out and hit[1] == B:
            call = self._calls
            self._calls = call + 1
            st = self._sample_entry(*hit[2][0], self._seed, call, self._raw_stream(self._dev_idx))
            if st:
                _lib.check(st, self._what)
            return out
        if out is not None and len(out['masks']) != B:
            raise ValueError(f"out= holds a batch of {len(out['masks'])} samples, not {B}")
        out, held, idx_t = self._batch(B, record_draws)
        dr, staged, rec, rec_t = self._stage(B, idxs, draws, record_draws)
        seed, call = self._next_seed()
        args = self._sample_args(held, dr, rec)
        st = self._sample_entry(*args, seed, call, self._raw_stream(self._dev_idx))
        _lib.check(st, self._what)
        del staged  # alive until the launch was issued
        if plain:
            # a refill's leading arguments (a plain call has neither draws nor
            # a record), and what keeps the descriptors alive
            self._remember(self._out_cache, out, B, (args, held))
        if record_draws:
            out.update(self._recorded(rec_t, idx_t))
        return out

    def _sample_visual(self, batch_size, idxs=None, draws=None, record_draws=False, out=None, evaluation=False):
        """sample() of a buffer with ``frame_stack`` or a live ``p_aug``
        (``GCDataset._sample_visual`` for the ring): the coin, the sample
        launch over the non-image columns with its index outputs requested,
        then one ogbx_online_visual_gather launch over the image columns.  An
        ``out=`` refill issues the same two launches and draws the same coin."""
        torch = _torch()
        B = int(batch_size)
        if self._steps == 0:
            raise ValueError(f'cannot sample from an empty {self._NAME}')
        crop = bool(self._p_aug_live and not evaluation and np.random.rand() < self._p_aug)
        draws = dict(draws or {})
        crop_from = draws.pop('crop_from', None)
        cf = self._stage_crop_from(crop_from, B) if (crop and crop_from is not None and self._visual) else None
        plain = idxs is None and not draws and crop_from is None and not record_draws
        if self._out_gen != self._gen:  # a column was replaced
            self._vis_cache.clear()
            self._out_gen = self._gen
        hit = self._vis_cache.get(id(out)) if (out is not None and plain) else None
        if hit is not None and hit[0] is out and hit[1] == B:
            st = hit[2]
        else:
            if out is not None and len(out['masks']) != B:
                raise ValueError(f"out= holds a batch of {len(out['masks'])} samples, not {B}")
            vcols = [] if self._visual else None
            out, held, idx_t = self._batch(B, True, vcols)
            nv = len(vcols or ())
            if nv > REPLAY_MAX_COLS:  # OGBX_VISUAL_MAX_COLS
                raise ValueError(f'at most {REPLAY_MAX_COLS} image columns per sample, got {nv}')
            varr = (OnlineVisualColumn * max(1, nv))(*(vcols or ()))
            st = (held, varr, nv, self._visual_indices(idx_t), idx_t)
            if plain:
                self._remember(self._vis_cache, out, B, st)
        held, varr, nv, vidx, idx_t = st
        dr, staged, rec, rec_t = self._stage(B, idxs, draws, record_draws)
        seed, call = self._next_seed()
        stream = self._raw_stream(self._dev_idx)
        _lib.check(self._sample_entry(*self._sample_args(held, dr, rec), seed, call, stream), self._what)
        cf_out = None
        if nv:
            if crop and record_draws:
                cf_out = torch.empty((B, 2), dtype=torch.int64, device=self.device)
            _lib.check(self._Lv.ogbx_online_visual_gather(
                self._ring, self._hcfg_ptr(), varr, nv, B, vidx, self._frame_stack or 1, CROP_PADDING, _lib.ptr(cf),
                int(crop and cf is None), seed, call, _lib.ptr(cf_out), stream), 'online_visual_gather')
        del staged, cf  # alive until the launches were issued
        if record_draws:
            out.update(self._recorded(rec_t, idx_t, crop_from=cf_out))
        return out

    # --------------------------------------------------------------- TRL batches
    # what the TRL branch adds (datasets.py:261-276) to the four RESERVED keys of a GC batch
    _TRL_KEYS = tuple(k for k, _, _ in _TRL_LAYOUT[4:])

    def _init_trl(self):
        """What a buffer with a TRL agent name adds at construction: the
        config checks, the prefix table ``P`` with its scan storage, the
        counter of bad samples, and ``sample`` bound to ``_sample_trl``."""
        torch = _torch()
        if not self._TRL_OK:
            raise NotImplementedError(f'{self._NAME}.sample has no TRL branch (nor has the reference\'s HGCDataset)')
        if self.config['value_p_curgoal'] != 0 or self.config['value_p_randomgoal'] != 0:
            raise ValueError(_TRL_VALUE_GOALS)
        if self._frame_stack is not None or self._p_aug_live:
            raise NotImplementedError('TRL batches over the ring are not implemented for visual buffers: the config '
                                      'has frame_stack or a live p_aug (p_aug > 0)')
        if 'actions' not in self:
            raise ValueError("a TRL GCReplayBuffer needs an 'actions' column")
        bad = [k for k in self if k in self._TRL_KEYS]
        if bad:
            raise ValueError(f'a TRL GCReplayBuffer cannot have columns named {bad}: sample() returns keys of these '
                             f'names')
        L = self._Lt = _online_trl.bind()
        need = ctypes.c_size_t(0)
        _lib.check(L.ogbx_online_trl_table_bytes(self.num_envs, ctypes.byref(need)), 'online_trl_table_bytes')
        self._trl_P = torch.zeros(self.num_envs + 1, dtype=torch.int64, device=self.device)
        self._trl_tmp = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        self._trl_bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._trl_built = None  # (steps, clears, stream) P was built for
        self.trl_table_builds = 0  # launches of the table scan so far
        self.sample = self._sample_trl

    def trl_bad_samples(self):
        """Samples of Philox calls so far that had no row between the sample
        and its value goal (one read of the device counter).  Nonzero only
        when every live row ended an episode at the time of a call."""
        return int(self._trl_bad.item())

    def _trl_batch(self, B, record, checked):
        """A new TRL batch (``_trl_walk``): the output dict, what a refill
        passes on (the column descriptors, selectors 0..4, and the scalar
        outputs), the index outputs and the counter of a checked call."""
        out, cols, outs, idx_t, bad = self._trl_walk(B, record, checked)
        arr = (GcColumn * len(cols))(*cols)  # at most 14 columns of the buffer and 8 further gathers
        return out, (arr, len(cols), outs), idx_t, bad

    def _sample_trl(self, batch_size, idxs=None, draws=None, record_draws=False, out=None, evaluation=False):
        """sample() of a buffer whose config has a TRL agent name
        (datasets.py:213-276 over the snapshot): the prefix table of the pick
        counts is rebuilt when ``steps`` (or ``clear()``, or the stream)
        changed since it was built -- one scan, ``ogbx_online_trl_table`` --
        then ONE launch of ``online_trl_sample_kernel``
        (``ogbx_online_trl_sample``, include/ogbx_online_trl.h).  Arguments as
        ``sample``; ``draws`` also takes ``'midpoint'``, the rows of the
        reference's ``randint(idxs, value_goal_idxs)``, and its ``pick`` /
        ``a_pick`` index the pick table (every live row that is not the last
        of its trajectory, in snapshot order).  Needs ``steps >= 2``."""
        torch = _torch()
        B = int(batch_size)
        if self._steps < 2:
            if self._steps == 0:
                raise ValueError(f'cannot sample from an empty {self._NAME}')
            raise ValueError(f'a TRL batch needs steps >= 2: the one live step of every env is the last row of its '
                             f'trajectory, so no row can be picked')
        draws = dict(draws or {})
        midpoint = draws.pop('midpoint', None)
        mid_in = self._stage_midpoint(midpoint, B) if midpoint is not None else None
        checked = idxs is not None or bool(draws) or mid_in is not None  # as GCDataset._sample_trl
        plain = not checked and not record_draws
        if self._out_gen != self._gen:  # a column was replaced
            self._out_cache.clear()
            self._out_gen = self._gen
        hit = self._out_cache.get(id(out)) if (out is not None and plain) else None
        idx_t, bad = {}, None
        if hit is not None and hit[0] is out and hit[1] == B:
            held = hit[2]
        else:
            if out is not None and len(out['masks']) != B:
                raise ValueError(f"out= holds a batch of {len(out['masks'])} samples, not {B}")
            out, held, idx_t, bad = self._trl_batch(B, record_draws, checked)
            if plain:
                self._remember(self._out_cache, out, B, held)
        arr, ncols, outs = held
        dr, staged, rec, rec_t = self._stage(B, idxs, draws, record_draws)
        mid_rec = torch.empty(B, dtype=torch.int64, device=self.device) if record_draws else None
        seed, call = self._next_seed()
        stream = self._raw_stream(self._dev_idx)
        L = self._Lt
        built = (self._steps, self._clears, stream)
        if built != self._trl_built:
            _lib.check(L.ogbx_online_trl_table(self._ring, self._trl_P.data_ptr(), self._trl_tmp.data_ptr(),
                                               self._trl_tmp.numel(), stream), 'online_trl_table')
            self._trl_built = built
            self.trl_table_builds += 1
        _lib.check(L.ogbx_online_trl_sample(self._ring, self._trl_P.data_ptr(), self._cfg, arr, ncols, B, dr,
                                            _lib.ptr(mid_in), seed, call, outs, rec, _lib.ptr(mid_rec), stream),
                   'online_trl_sample')
        del staged, mid_in  # alive until the launch was issued
        if bad is not None:
            self._check_bad(bad, B, 'online_trl_sample')
        if record_draws:
            out.update(self._recorded(rec_t, idx_t, midpoint=mid_rec))
        return out

    # --------------------------------------------------------------- ATC batches
    atc_table_builds = 0  # launches of the ATC table build so far (the first sample_atc makes it the instance's)
    # _atc_bad: the device counter of sample_atc's unchecked calls, from its first call on

    def _init_atc(self):
        """What the first ``sample_atc`` allocates: the segment table ``W``,
        the prefix table ``P``, the storage of the table build and the counter
        of bad samples.  A buffer that never draws ATC pairs holds none."""
        torch = _torch()
        pad = int(self.config.get('augment_padding', ATC_CROP_PADDING))
        if pad < 0:
            raise ValueError(f'augment_padding must be >= 0, got {pad}')
        L = _online_atc.bind()
        need = ctypes.c_size_t(0)
        _lib.check(L.ogbx_online_atc_table_bytes(self.num_envs, ctypes.byref(need)), 'online_atc_table_bytes')
        self._atc_pad = pad
        self._atc_W = torch.zeros(self.horizon, self.num_envs, dtype=torch.int32, device=self.device)
        self._atc_P = torch.zeros(self.num_envs + 1, dtype=torch.int64, device=self.device)
        self._atc_tmp = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        # allocated once and never replaced: the out= cache holds its address (the refill's AtcOutputs)
        self._atc_bad = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._atc_built = None  # (steps, clears, stream, k) W and P were built for
        self._atc_cache = {}
        self._atc_gen = self._gen
        self._La = L

    def atc_bad_samples(self):
        """Samples of ``sample_atc``'s Philox calls so far that found valid(k)
        empty (one read of the device counter): nonzero only when every live
        episode was shorter than k + 1 at the time of a call."""
        return int(self._atc_bad.item()) if self._atc_bad is not None else 0

    # what _AtcHost asks for
    _atc_out_strict = True
    _atc_pick_checked = True
    _atc_bad_rows = ('online_atc_sample: {n} of {B} samples have idx + k (k={k}) past the end of their episode, or '
                     'idx outside the snapshot')

    def _atc_source(self):
        return self._column_of('observations', self.rows)

    def _atc_build(self, k, stream, built):
        """W and P of valid(k) for ``built`` = (steps, clears, stream, k)."""
        _lib.check(self._La.ogbx_online_atc_table(self._ring, k, self._atc_W.data_ptr(), self._atc_P.data_ptr(),
                                                  self._atc_tmp.data_ptr(), self._atc_tmp.numel(), stream),
                   'online_atc_table')
        self._atc_built = built
        self.atc_table_builds += 1

    def _atc_launch(self, stream, col, B, k, ix, pk, cf, draw, seed, call, outs):
        built = (self._steps, self._clears, stream, k)
        if built != self._atc_built:
            self._atc_build(k, stream, built)
        _lib.check(self._La.ogbx_online_atc_sample(
            self._ring, k, self._atc_W.data_ptr(), self._atc_P.data_ptr(), col, B, self._frame_stack or 1,
            self._atc_pad, _lib.ptr(ix), _lib.ptr(pk), _lib.ptr(cf), draw, seed, call, outs, stream),
            'online_atc_sample')

    def sample_atc(self, batch_size, k, evaluation=False, idxs=None, draws=None, record_draws=False, out=None):
        """ATCDataset.sample(batch_size, k) (datasets.py:401-415) over the
        snapshot without its ``next_observations``: ``observations`` at the
        anchors and ``positive_observations`` k steps later in the same
        episode, both from the ``observations`` column, stacked by the
        config's ``frame_stack`` as a visual ``sample`` stacks (an episode
        whose head was overwritten starts at its oldest live row) and, when
        the call's coin comes up (``p_aug``, GCDataset's rule), cropped with
        one ``(cy, cx)`` per sample at padding ``augment_padding`` (default
        4).  Every live row is a candidate.

        valid(k) changes with every insert and is never built: the buffer
        keeps ``W`` (per env, the anchors before each live episode) and ``P``
        (their prefix sum over envs) and rebuilds both when ``steps``, the
        count of ``clear()`` calls, the stream or ``k`` changed since the last
        build (``ogbx_online_atc_table``; ``atc_table_builds`` counts), then
        issues ONE launch of ``online_atc_sample_kernel``
        (``ogbx_online_atc_sample``, include/ogbx_online_atc.h).  All of it is
        allocated by the first call.

        k: the temporal offset, an int >= 0; ``k >= live_steps`` raises the
        reference's ValueError.  A valid(k) that is empty because every live
        episode is shorter than k + 1 is not read back: the Philox path counts
        its samples in ``atc_bad_samples()``.
        idxs: explicit flat rows; those that leave the snapshot or whose
        idx + k leaves their episode raise ValueError with their count (one
        read-back).
        draws: ``'pick'`` (positions into valid(k), snapshot order) and
        ``'crop_from'`` ([batch_size, 2], used when the call crops).
        record_draws: adds ``_idxs`` (flat rows) and ``_draws``.
        out: a batch of an earlier plain call with the same batch_size,
        refilled in place (stream ordered); k may differ between the calls.
        Seeds and calls come from the buffer's one counter."""
        B, k = int(batch_size), operator.index(k)
        if k < 0:
            raise ValueError(f'k must be >= 0, got {k}')
        if self._steps == 0:
            raise ValueError(f'cannot sample from an empty {self._NAME}')
        if k >= self.live_steps:  # no episode holds k + 1 live rows
            raise ValueError(f'No valid ATC indices found for k={k}.')
        if self._atc_bad is None:
            self._init_atc()
        # the coin stays on the host (datasets.py:411-412); the offsets are device draws
        crop = bool(self._p_aug_live and not evaluation and np.random.rand() < self._p_aug)
        if self._atc_gen != self._gen:  # a column was replaced
            self._atc_cache.clear()
            self._atc_gen = self._gen
        # the conservative form of _atc_call's plain rule: a draws dict that holds only None goes there
        plain = idxs is None and not draws and not record_draws
        hit = self._atc_cache.get(id(out)) if (out is not None and plain) else None
        stream = self._raw_stream(self._dev_idx)
        if hit is None or hit[0] is not out or hit[1] != B:
            return self._atc_call(B, k, crop, idxs, draws, record_draws, out, stream)
        seed, call = self._next_seed()
        built = (self._steps, self._clears, stream, k)
        if built != self._atc_built:
            self._atc_build(k, stream, built)
        _lib.check(self._La.ogbx_online_atc_sample(
            self._ring, k, self._atc_W.data_ptr(), self._atc_P.data_ptr(), hit[2], B, self._frame_stack or 1,
            self._atc_pad, None, None, None, int(crop), seed, call, hit[3], stream), 'online_atc_sample')
        return out

    # ------------------------------------- what HGCReplayBuffer supplies instead
    # (with _batch; the hook names of GCDataset / HGCDataset where they match)
    _NAME = 'GCReplayBuffer'  # names the class in sample()'s message
    _what = 'online_gc_sample'  # names the call in error messages

    def _sample_args(self, held, dr, rec):
        """The arguments of ``_sample_entry`` before (seed, call, stream), from
        what ``_batch`` returned second."""
        return self._ring, self._cfg, held[0], dr, rec

    def get_subset(self, idxs):
        return self.sample(len(idxs), idxs=idxs)

    def get_random_idxs(self, num_idxs):
        """Uniform flat rows of the snapshot."""
        return self.sample(num_idxs, record_draws=True)['_idxs']

    # ----------------------------------------------------------------- snapshot
    def snapshot(self):
        """The live rows as a ``Dataset`` in the OGBench layout: every column
        unrolled env-major (row ``e * L + k`` = env e at step ``S - L + k``)
        plus ``terminals`` (float32): 1 on the last row of every closed episode
        and on every env's newest row.  Built with torch ops (not a hot path):
        for tests, and for saving collected data."""
        torch = _torch()
        S, T, N, L = self._steps, self.horizon, self.num_envs, self.live_steps
        if S == 0:
            raise ValueError('an empty GCReplayBuffer has no snapshot')
        slots = torch.arange(S - L, S, dtype=torch.int64, device=self.device) % T  # [L]
        rows = (slots[None, :] * N + torch.arange(N, dtype=torch.int64, device=self.device)[:, None]).reshape(-1)
        data = {k: v.index_select(0, rows) for k, v in self.items()}
        seq = self.ep_seq.reshape(-1).index_select(0, rows).reshape(N, L)
        term = torch.ones(N, L, dtype=torch.float32, device=self.device)
        term[:, :-1] = (seq[:, 1:] != seq[:, :-1]).to(torch.float32)  # the next live row belongs to another episode
        data['terminals'] = term.reshape(-1)
        return Dataset(data, device=self.device)


class HGCReplayBuffer(_HgcHost, GCReplayBuffer):
    """Hierarchical hindsight sampling over the episode ring of
    ``GCReplayBuffer``: the same constructor, inserts, ``clear``, ``snapshot``
    and state, and a ``sample`` that returns what the reference's
    ``HGCDataset.sample`` (datasets.py:496-643) returns over the snapshot
    (include/ogbx_online_hgc.h).

    The config also reads ``subgoal_steps`` and the optional
    ``high_subgoal_steps``, ``value_subgoal_steps``, ``actor_subgoal_steps``,
    ``low_subgoal_steps`` and ``low_discount``, resolved as
    ``HGCDataset.__init__`` resolves them.

    ``sample`` is ONE launch of ``online_hgc_sample_kernel`` and returns, bit
    for bit, ``HGCDataset(Dataset(snapshot), config).sample`` under the same
    draws -- with the Philox draws at one ``(seed, call)`` too -- for the
    buffer's own keys followed by ``high_value_reps`` ..
    ``low_actor_next_observations`` in the reference's order, with its aliases
    (``high_value_reps is observations``, ``value_goals is high_value_goals``,
    ``high_actor_targets is high_actor_actions``).  The goal-type keys come
    from ``oracle_reps`` when the buffer has that column, else from
    ``observations``.  Every index it takes or reports is a flat index of the
    snapshot.  Nothing is read back.

    As a visual buffer (``frame_stack`` / ``p_aug``, see ``GCReplayBuffer``)
    it stacks ``observations``, ``next_observations`` and the goal / "action"
    / next-observation keys of ``HGCDataset._VISUAL_KEYS`` (the goal-type ones
    only without ``oracle_reps``) and crops the keys of
    ``HGCDataset._CROP_KEYS``: ``high_value_reps`` -- then a tensor of its own
    -- and ``low_value_goals`` stay uncropped.  ``sample`` is then two
    launches, ``online_hgc_sample_kernel`` and ``online_visual_gather_kernel``.
    """

    _HGC_KEYS = tuple(k for k, _, _ in _HGC_LAYOUT if k not in GCReplayBuffer.RESERVED)
    RESERVED = GCReplayBuffer.RESERVED + _HGC_KEYS
    MAX_SAMPLE_COLS = 32  # kGcMaxCols

    def __init__(self, data, num_envs, horizon, config, device=None, seed=None):
        super().__init__(data, num_envs, horizon, config, device=device, seed=seed)
        self._sample_entry = self._L.ogbx_online_hgc_sample
        self._init_hgc(config)
        if min(self.value_subgoal_steps, self.actor_subgoal_steps, self.low_subgoal_steps) < 1:
            raise ValueError('subgoal steps must be >= 1')

    # sample() is GCReplayBuffer's; what differs for the hierarchical sampler
    # (with the hooks of _HgcHost):
    _NAME = 'HGCReplayBuffer'
    _what = 'online_hgc_sample'

    def _batch(self, B, record, vcols=None):
        out, cols, outs, idx_t = self._hgc_walk(B, record, vcols)
        if len(cols) > self.MAX_SAMPLE_COLS:
            raise ValueError(f'at most {self.MAX_SAMPLE_COLS} columns per sample, got {len(cols)}')
        arr = (GcColumn * len(cols))(*cols)
        return out, (arr, len(cols), B, outs), idx_t

    def _sample_args(self, held, dr, rec):
        arr, ncols, B, outs = held
        return self._ring, self._cfg, self._hcfg, arr, ncols, B, dr, outs, rec
