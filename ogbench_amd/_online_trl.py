"""ctypes binding of include/ogbx_online_trl.h (exported by libogbx.so): TRL
batches over the episode ring, behind a TRL ``agent_name`` in the config of
``GCReplayBuffer``."""

from __future__ import annotations

import ctypes

from . import _lib

ONLINE_TRL_API_VERSION = 1  # OGBX_ONLINE_TRL_API_VERSION
ONLINE_TRL_TABLE_TILE = 2048  # OGBX_ONLINE_TRL_TABLE_TILE


def bind():
    """libogbx with the signatures of include/ogbx_online_trl.h declared."""
    L = _lib.lib()
    if not getattr(L, '_online_trl_bound', False):
        from . import datasets as D  # the ring, config, draw and output structs live with the samplers

        P, vp = ctypes.POINTER, ctypes.c_void_p
        L.ogbx_online_trl_api_version.restype = ctypes.c_int32
        L.ogbx_online_trl_api_version.argtypes = []
        L.ogbx_online_trl_table_bytes.restype = ctypes.c_int32
        L.ogbx_online_trl_table_bytes.argtypes = [ctypes.c_int64, P(ctypes.c_size_t)]
        L.ogbx_online_trl_table.restype = ctypes.c_int32
        L.ogbx_online_trl_table.argtypes = [P(D.OnlineRing), vp, vp, ctypes.c_size_t, vp]
        L.ogbx_online_trl_sample.restype = ctypes.c_int32
        L.ogbx_online_trl_sample.argtypes = [
            P(D.OnlineRing), vp, P(D.GcConfig), vp, ctypes.c_int32, ctypes.c_int64, P(D.GcDraws), vp,
            ctypes.c_uint64, ctypes.c_uint64, P(D.TrlOutputs), P(D.GcDrawRecord), vp, vp,
        ]
        if L.ogbx_online_trl_api_version() != ONLINE_TRL_API_VERSION:
            raise RuntimeError(f'{_lib.LIB_PATH} has online-TRL API version {L.ogbx_online_trl_api_version()}, '
                               f'this package binds {ONLINE_TRL_API_VERSION}; rebuild it (make -C ogbench_amd/csrc)')
        L._online_trl_bound = True
    return L
