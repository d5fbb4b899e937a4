"""ctypes binding of include/ogbx_online_visual.h (exported by libogbx.so):
frame stacks and random crops over the episode ring, behind the ``frame_stack``
and ``p_aug`` config keys of ``GCReplayBuffer`` / ``HGCReplayBuffer``."""

from __future__ import annotations

import ctypes

from . import _lib

ONLINE_VISUAL_API_VERSION = 1  # OGBX_ONLINE_VISUAL_API_VERSION


class OnlineVisualColumn(ctypes.Structure):
    """ogbx_online_visual_column."""
    _fields_ = [
        ('src', ctypes.c_void_p),
        ('alt', ctypes.c_void_p),
        ('dst', ctypes.c_void_p),
        ('height', ctypes.c_int32),
        ('width', ctypes.c_int32),
        ('px_bytes', ctypes.c_int32),
        ('select', ctypes.c_int32),
        ('stack', ctypes.c_int32),
        ('crop', ctypes.c_int32),
    ]


def bind():
    """libogbx with the signatures of include/ogbx_online_visual.h declared."""
    L = _lib.lib()
    if not getattr(L, '_online_visual_bound', False):
        from . import datasets as D  # the ring, config and index structs live with the samplers

        P, vp = ctypes.POINTER, ctypes.c_void_p
        L.ogbx_online_visual_api_version.restype = ctypes.c_int32
        L.ogbx_online_visual_api_version.argtypes = []
        L.ogbx_online_visual_gather.restype = ctypes.c_int32
        L.ogbx_online_visual_gather.argtypes = [
            P(D.OnlineRing), P(D.HgcConfig), vp, ctypes.c_int32, ctypes.c_int64, P(D.VisualIndices),
            ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, vp, vp,
        ]
        if L.ogbx_online_visual_api_version() != ONLINE_VISUAL_API_VERSION:
            raise RuntimeError(f'{_lib.LIB_PATH} has online-visual API version {L.ogbx_online_visual_api_version()}, '
                               f'this package binds {ONLINE_VISUAL_API_VERSION}; rebuild it (make -C ogbench_amd/csrc)')
        L._online_visual_bound = True
    return L
