"""ctypes binding of include/ogbx_play.h (exported by libogbx.so): the
data-collection reset of the powderworld envs and the play policy's action
plan.  ``plan`` is the one-launch plan as a function of tensors."""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

POWDER_MODE_DATA = 1  # OGBX_POWDER_MODE_DATA
PLAY_API_VERSION = 1  # OGBX_PLAY_API_VERSION
KINDS = ('fill', 'line', 'square')
WEIGHTS = (1.0, 3.0, 3.0)  # generate_powderworld.py:40


class PlayConfig(ctypes.Structure):
    _fields_ = [
        ('size', ctypes.c_int32),
        ('num_elems', ctypes.c_int32),
        ('xy_size', ctypes.c_int32),
        ('pad', ctypes.c_int32),
        ('p_random', ctypes.c_double),
        ('cdf', ctypes.c_double * 3),
        ('env_base', ctypes.c_int64),
        ('episode', ctypes.c_int64),
    ]


class PlayTape(ctypes.Structure):
    _fields_ = [('tape', ctypes.c_void_p), ('tape_len', ctypes.c_int64), ('short_count', ctypes.c_void_p)]


class PlayOutputs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('used', 'decisions', 'terminals')]


def bind():
    """libogbx with the signatures of include/ogbx_play.h declared."""
    L = _lib.lib()
    if not getattr(L, '_play_bound', False):
        P, vp = ctypes.POINTER, ctypes.c_void_p
        L.ogbx_play_api_version.restype = ctypes.c_int32
        L.ogbx_play_api_version.argtypes = []
        L.ogbx_play_powder_reset.restype = ctypes.c_int32
        L.ogbx_play_powder_reset.argtypes = [vp, vp, vp, ctypes.c_uint64, vp]
        L.ogbx_play_plan.restype = ctypes.c_int32
        L.ogbx_play_plan.argtypes = [P(PlayConfig), ctypes.c_int64, ctypes.c_int32, vp, P(PlayTape), P(PlayOutputs),
                                     ctypes.c_uint64, vp]
        L.ogbx_play_sample_semantic.restype = ctypes.c_int32
        L.ogbx_play_sample_semantic.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_uint64, ctypes.c_uint64, vp, vp]
        if L.ogbx_play_api_version() != PLAY_API_VERSION:
            raise RuntimeError(f'{_lib.LIB_PATH} has play API version {L.ogbx_play_api_version()}, this package '
                               f'binds {PLAY_API_VERSION}; rebuild it (make -C ogbench_amd/csrc)')
        L._play_bound = True
    return L


def behavior_cdf(weights=WEIGHTS):
    """The cdf np.random.choice(agents, p=weights / sum) searches: cumsum of the
    normalised weights, divided by its last entry (float64, as NumPy does)."""
    p = np.asarray(weights, np.float64)
    if p.shape != (3,) or not np.all(p >= 0) or not p.sum() > 0:
        raise ValueError('weights must be three non-negative numbers with a positive sum (fill, line, square)')
    cdf = (p / p.sum()).cumsum()
    cdf /= cdf[-1]
    return cdf


def plan(num_envs, T, *, size, num_elems, xy_size, p_random_action=0.5, weights=WEIGHTS, seed=0, episode=0,
         env_base=0, tape=None, device=None, records=False):
    """The play policy's actions of one episode of every env, in one launch.

    Returns a dict: ``actions`` int32 [T, N] (step major, what ``rollout``
    takes), ``terminals`` bool [T] and ``used`` int32 [N] (draws consumed); with
    ``records`` also ``decisions`` int32 [(T + 2) // 3, N] (bit 0 random, bits
    1-2 behaviour kind, bit 3 freshly chosen, bits 8.. index in the sequence).
    tape: float64 [N, L] of injected draws (include/ogbx_play.h), else Philox
    keyed by (seed, env_base + e, episode).  Raises ValueError if a tape runs out.
    """
    import torch

    from .locomaze import _resolve_device

    dev = _resolve_device(device)
    L = bind()
    N, T = int(num_envs), int(T)
    if N <= 0 or T <= 0:
        raise ValueError(f'num_envs and T must be positive, got {N} and {T}')
    if not 0.0 <= float(p_random_action) <= 1.0:
        raise ValueError(f'p_random_action must be in [0, 1], got {p_random_action}')
    cfg = PlayConfig(size=int(size), num_elems=int(num_elems), xy_size=int(xy_size), p_random=float(p_random_action),
                     cdf=(ctypes.c_double * 3)(*behavior_cdf(weights)), env_base=int(env_base), episode=int(episode))
    out = dict(actions=torch.empty(T, N, dtype=torch.int32, device=dev),
               terminals=torch.empty(T, dtype=torch.bool, device=dev),
               used=torch.empty(N, dtype=torch.int32, device=dev))
    if records:
        out['decisions'] = torch.empty((T + 2) // 3, N, dtype=torch.int32, device=dev)
    tp, short = None, None
    if tape is not None:
        tape = torch.as_tensor(tape).to(dev, torch.float64).contiguous()
        if tape.dim() != 2 or tape.shape[0] != N or tape.shape[1] < 1:
            raise ValueError(f'tape must be float64 [{N}, L >= 1], got {tuple(tape.shape)}')
        short = torch.zeros(1, dtype=torch.int64, device=dev)
        tp = PlayTape(tape.data_ptr(), tape.shape[1], short.data_ptr())
    o = PlayOutputs(out['used'].data_ptr(), out['decisions'].data_ptr() if records else None,
                    out['terminals'].data_ptr())
    with torch.cuda.device(dev):
        _lib.check(L.ogbx_play_plan(cfg, N, T, _lib.ptr(out['actions']), tp, o, int(seed) & ((1 << 64) - 1),
                                    _lib.stream_of(dev)), 'plan')
    if short is not None:
        out['short_count'] = short
        n_short = int(short.item())
        if n_short:
            err = ValueError(f'plan: the tape of {n_short} env(s) ran out (tape_len {tape.shape[1]})')
            err.short_count = n_short
            raise err
    return out
