"""ctypes binding of include/ogbx_online_atc.h (exported by libogbx.so): ATC
batches over the episode ring, behind ``GCReplayBuffer.sample_atc``."""

from __future__ import annotations

import ctypes

from . import _lib

ONLINE_ATC_API_VERSION = 1  # OGBX_ONLINE_ATC_API_VERSION
ONLINE_ATC_TABLE_TILE = 2048  # OGBX_ONLINE_ATC_TABLE_TILE


def bind():
    """libogbx with the signatures of include/ogbx_online_atc.h declared."""
    L = _lib.lib()
    if not getattr(L, '_online_atc_bound', False):
        from . import datasets as D  # the ring, column and output structs live with the samplers

        P, vp = ctypes.POINTER, ctypes.c_void_p
        L.ogbx_online_atc_api_version.restype = ctypes.c_int32
        L.ogbx_online_atc_api_version.argtypes = []
        L.ogbx_online_atc_table_bytes.restype = ctypes.c_int32
        L.ogbx_online_atc_table_bytes.argtypes = [ctypes.c_int64, P(ctypes.c_size_t)]
        L.ogbx_online_atc_table.restype = ctypes.c_int32
        L.ogbx_online_atc_table.argtypes = [P(D.OnlineRing), ctypes.c_int64, vp, vp, vp, ctypes.c_size_t, vp]
        L.ogbx_online_atc_sample.restype = ctypes.c_int32
        L.ogbx_online_atc_sample.argtypes = [
            P(D.OnlineRing), ctypes.c_int64, vp, vp, P(D.AtcColumn), ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
            vp, vp, vp, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, P(D.AtcOutputs), vp,
        ]
        if L.ogbx_online_atc_api_version() != ONLINE_ATC_API_VERSION:
            raise RuntimeError(f'{_lib.LIB_PATH} has online-ATC API version {L.ogbx_online_atc_api_version()}, '
                               f'this package binds {ONLINE_ATC_API_VERSION}; rebuild it (make -C ogbench_amd/csrc)')
        L._online_atc_bound = True
    return L
