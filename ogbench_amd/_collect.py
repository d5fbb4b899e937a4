"""ctypes binding of include/ogbx_collect.h (exported by libogbx.so): the fused
point-maze collector behind ``MazeEnv.collect``."""

from __future__ import annotations

import ctypes

from . import _lib

COLLECT_ABI_VERSION = 1  # OGBX_COLLECT_ABI_VERSION
MODES = {'path': 0, 'navigate': 1, 'stitch': 2, 'explore': 3}  # OGBX_COLLECT_*
EXPLORE_PERIOD = 10  # generate_locomaze.py:150
TAPE_KEYS = ('normal', 'goal_pick', 'goal_noise', 'dir')
COLUMNS = ('observations', 'actions', 'terminals', 'qpos')


class CollectConfig(ctypes.Structure):
    _fields_ = [
        ('mode', ctypes.c_int32),
        ('explore_period', ctypes.c_int32),
        ('noise', ctypes.c_double),
        ('goal_cells', ctypes.c_void_p),
        ('n_goal_cells', ctypes.c_int32),
        ('pad', ctypes.c_int32),
    ]


class CollectTape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in TAPE_KEYS] + [('steps', ctypes.c_int64)]


class CollectOutputs(ctypes.Structure):
    _fields_ = ([(k, ctypes.c_void_p) for k in COLUMNS] + [('row_stride', ctypes.c_int64), ('row_offset', ctypes.c_int64)]
                + [(k, ctypes.c_void_p) for k in ('qpos64', 'goal64', 'success')])


def bind():
    """libogbx with the signatures of include/ogbx_collect.h declared."""
    L = _lib.lib()
    if not getattr(L, '_collect_bound', False):
        P, vp = ctypes.POINTER, ctypes.c_void_p
        L.ogbx_collect_abi_version.restype = ctypes.c_int32
        L.ogbx_collect_abi_version.argtypes = []
        L.ogbx_maze_collect.restype = ctypes.c_int32
        L.ogbx_maze_collect.argtypes = [vp, P(CollectConfig), P(CollectTape), ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_uint64, P(CollectOutputs), vp]
        if L.ogbx_collect_abi_version() != COLLECT_ABI_VERSION:
            raise RuntimeError(f'{_lib.LIB_PATH} has collect ABI version {L.ogbx_collect_abi_version()}, this '
                               f'package binds {COLLECT_ABI_VERSION}; rebuild it (make -C ogbench_amd/csrc)')
        L._collect_bound = True
    return L


def tape_shapes(steps, num_envs, period=EXPLORE_PERIOD):
    """The shape of every tape entry for a tape of `steps` episode steps."""
    T, N = int(steps), int(num_envs)
    return dict(normal=(T, N, 2), goal_pick=(T, N), goal_noise=(T, N, 2), dir=(-(-T // period), N, 2))


def check_tape(tape, num_envs, period=EXPLORE_PERIOD):
    """Validate a tape dict (entries optional) without touching a device;
    returns the episode steps it covers (0 for an empty tape)."""
    import numpy as np

    if tape is None:
        return 0
    if not isinstance(tape, dict) or any(k not in TAPE_KEYS for k in tape):
        raise ValueError(f'tape must be a dict with keys among {TAPE_KEYS}')
    steps = None
    for k in ('normal', 'goal_pick', 'goal_noise'):
        if tape.get(k) is not None:
            s = int(np.shape(tape[k])[0]) if np.ndim(tape[k]) else -1
            if steps is not None and s != steps:
                raise ValueError(f'tape entries disagree on the number of steps ({steps} and {s})')
            steps = s
    if steps is None and tape.get('dir') is not None:
        steps = (int(np.shape(tape['dir'])[0]) if np.ndim(tape['dir']) else -1) * period
    if steps is None:
        return 0
    want = tape_shapes(steps, num_envs, period)
    for k in TAPE_KEYS:
        if tape.get(k) is not None and tuple(np.shape(tape[k])) != want[k]:
            raise ValueError(f'tape[{k!r}] must have shape {want[k]}, got {tuple(np.shape(tape[k]))}')
    return steps
