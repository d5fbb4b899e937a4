"""ctypes binding of include/ogbx_framestack.h (exported by libogbx.so): frame
stacks of batched env observations, behind ``wrappers.FrameStack``."""

from __future__ import annotations

import ctypes

from . import _lib

FRAMESTACK_ABI_VERSION = 1  # OGBX_FRAMESTACK_ABI_VERSION


class FrameStackShape(ctypes.Structure):
    _fields_ = [
        ('n', ctypes.c_int64),
        ('pixels', ctypes.c_int64),
        ('elem_bytes', ctypes.c_int64),
        ('num_stack', ctypes.c_int32),
        ('pad', ctypes.c_int32),
    ]


def bind():
    """libogbx with the signatures of include/ogbx_framestack.h declared."""
    L = _lib.lib()
    if not getattr(L, '_framestack_bound', False):
        P, vp = ctypes.POINTER, ctypes.c_void_p
        L.ogbx_framestack_abi_version.restype = ctypes.c_int32
        L.ogbx_framestack_abi_version.argtypes = []
        L.ogbx_framestack_fill.restype = ctypes.c_int32
        L.ogbx_framestack_fill.argtypes = [P(FrameStackShape), vp, vp, vp, vp]
        L.ogbx_framestack_push.restype = ctypes.c_int32
        L.ogbx_framestack_push.argtypes = [P(FrameStackShape), vp, vp, vp, vp, vp, vp, vp, vp]
        if L.ogbx_framestack_abi_version() != FRAMESTACK_ABI_VERSION:
            raise RuntimeError(f'{_lib.LIB_PATH} has framestack ABI version {L.ogbx_framestack_abi_version()}, this '
                               f'package binds {FRAMESTACK_ABI_VERSION}; rebuild it (make -C ogbench_amd/csrc)')
        L._framestack_bound = True
    return L


def shape_of(frame, num_stack):
    """The FrameStackShape of a contiguous frame tensor [N, ..., C]: pixels =
    the product of the middle axes, elem_bytes = C * itemsize."""
    assert frame.dim() >= 2 and frame.is_contiguous(), 'frames are contiguous [N, ..., C] tensors'
    n, c = int(frame.shape[0]), int(frame.shape[-1])
    pixels = 1
    for d in frame.shape[1:-1]:
        pixels *= int(d)
    return FrameStackShape(n=n, pixels=pixels, elem_bytes=c * frame.element_size(), num_stack=int(num_stack), pad=0)


def _on(device):
    """Make `device` current for the call (the library checks its pointers
    against the current device)."""
    import torch

    return torch.cuda.device(device)


def fill(shape, obs, mask, stack):
    """ogbx_framestack_fill on torch tensors (mask: u8 / bool [N] or None)."""
    L = bind()
    with _on(stack.device):
        _lib.check(L.ogbx_framestack_fill(shape, _lib.ptr(obs), _lib.ptr(mask), _lib.ptr(stack),
                                          _lib.stream_of(stack.device)), 'framestack_fill')


def push(shape, obs, prev, terminated, truncated, final_obs, next, final_stack):
    """ogbx_framestack_push on torch tensors (None -> NULL)."""
    L = bind()
    with _on(next.device):
        _lib.check(L.ogbx_framestack_push(shape, _lib.ptr(obs), _lib.ptr(prev), _lib.ptr(terminated),
                                          _lib.ptr(truncated), _lib.ptr(final_obs), _lib.ptr(next),
                                          _lib.ptr(final_stack), _lib.stream_of(next.device)), 'framestack_push')
