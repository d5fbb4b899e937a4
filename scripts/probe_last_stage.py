"""Diagnostic: does any env's LAST lean stage (RK phase 3 of the last substep)
iterate its active set?  With the mask-trace build (OGBX_MASK_TRACE: per env
and lean stage the mask the stage started from and the one it settled on, bit
31 of the second word = not settled), the near-wall batch of
tests/last_stage_batch.py at N = 4,096 for its 8 steps -- or, with `bench`, the
bench states at N = 65,536, every 20th of 300 steps.  Since the last stage has
no solve its two words are the carried mask; a build that still solved there
shows start != settled on the envs whose last stage iterated.  Prints the
counts and LAST_STAGE_CLEAN when no env's last stage iterated while earlier
stages did (the trace is live); exit status 1 otherwise.
  OGBX_LIB=_abx/libogbx_masks.so python scripts/probe_last_stage.py [bench]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ogbench_amd  # noqa: E402
from ogbench_amd import _lib  # noqa: E402


def _trace(L, buf, n):
    torch.cuda.synchronize()
    _lib.check(L.ogbx_diag_mask_trace(buf))
    return np.frombuffer(buf, dtype=np.uint32).reshape(65536, 20, 2)[:n].copy()


def main():
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    assert hasattr(L, 'ogbx_diag_mask_trace'), 'not a mask-trace build'
    L.ogbx_diag_mask_trace.restype = ctypes.c_int
    L.ogbx_diag_mask_trace.argtypes = [ctypes.c_void_p]
    buf = (ctypes.c_uint32 * (65536 * 40))()
    traces = []
    if len(sys.argv) > 1 and sys.argv[1] == 'bench':
        import bench

        n = 65536
        env, acts = bench._maze_job(n, 0, n, 128, dev)
        views = list(acts.unbind(0))
        for i in range(300):
            env.step(views[i % 128])
            if i >= 100 and i % 20 == 0:
                traces.append(_trace(L, buf, n))
    else:
        from last_stage_batch import K, MAZE, near_wall_batch

        n = 4096
        q, acts, _ = near_wall_batch(n)
        env = ogbench_amd.MazeEnv('point', MAZE, num_envs=n, device=dev, auto_reset=True)
        env.reset(seed=5)
        sd = env.state_dict()
        sd['qpos'] = torch.tensor(q, device=dev)
        env.load_state_dict(sd)
        a = torch.tensor(acts, device=dev)
        for t in range(K):
            env.step(a[t])
            traces.append(_trace(L, buf, n))
    env.close()
    a = np.concatenate(traces)  # [samples * envs, 20, 2]
    start, end, unsettled = a[:, :, 0], a[:, :, 1] & 0x7FFFFFFF, (a[:, :, 1] >> 31) != 0
    it = (start != end) | unsettled
    it[:, 0] = unsettled[:, 0]  # stage 0 always runs its Newton step (start is the u = 0 mask)
    contact = ((a[:, :, 0] | a[:, :, 1]) != 0).any(1)
    res = dict(num_envs=n, samples=len(traces), contact_env_samples=int(contact.sum()),
               iterating_by_stage=[int(x) for x in it.sum(0)], unsettled_by_stage=[int(x) for x in unsettled.sum(0)],
               last_stage_iterating=int(it[:, 19].sum()), last_stage_unsettled=int(unsettled[:, 19].sum()),
               last_stage_differs_from_carried=int((end[:, 19] != end[:, 18]).sum()))
    print(json.dumps(res), flush=True)
    clean = res['last_stage_iterating'] == 0 and res['last_stage_differs_from_carried'] == 0 and it[:, 1:19].any()
    if clean:
        print('LAST_STAGE_CLEAN', flush=True)
    return 0 if clean else 1


if __name__ == '__main__':
    sys.exit(main())
