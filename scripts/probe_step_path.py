"""Diagnostic: where a wave of maze_step_kernel spends its life outside the
lean contact stages.  Bench setting (pointmaze-large, N envs, task i%5+1,
auto-reset, uniform actions, warmed); every 10th step of 300 is stamped.  Per
wave: s_memtime at the kernel's outer boundaries (point_physics.h
g_path_stamps); consecutive differences are the parts of its stamped lifetime
(entry to after the final stores), so the parts sum to it.  Reports the
median band of the contact waves (those that ran the lean loop) and their
slowest 1 % by lifetime, in s_memtime (shader clock) cycles, and the shader
clock itself: delta s_memtime / delta s_memrealtime x 100 MHz, median over the
contact waves of the last launch of 2 s of back-to-back steps.

Run with OGBX_LIB=_abx/libogbx_path.so built by
  scripts/build_maze_variant.sh path -DOGBX_STAGE_STAMPS=2
usage: probe_step_path.py [N] [out.json]
"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ogbench_amd import _lib  # noqa: E402

# part k runs from stamp k to stamp k + 1
PARTS = ['prologue_loads', 'barrier', 'role_frame_flags', 'lean_setup', 'first_stage', 'steady_stages',
         'bail_check', 'success_reward', 'reset_obs', 'final_stores']
OUTSIDE = [p for p in PARTS if p not in ('first_stage', 'steady_stages')]


def main():
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    L = _lib.lib()
    env, acts = bench._maze_job(n, 0, n, 128, dev)
    views = list(acts.unbind(0))
    nw = min((n + 63) // 64, 4096)
    buf = (ctypes.c_ulonglong * (4096 * 16))()
    stamps = []
    for i in range(300):
        stamp = i >= 100 and i % 10 == 0
        if stamp:
            torch.cuda.synchronize()
            _lib.check(L.ogbx_diag_path_stamps(buf))  # clear
        env.step(views[i % 128])
        if stamp:
            torch.cuda.synchronize()
            _lib.check(L.ogbx_diag_path_stamps(buf))
            stamps.append(np.frombuffer(buf, dtype=np.uint64).reshape(4096, 16)[:nw, :11].astype(np.int64))
    t = np.concatenate(stamps)
    ran = (t[:, 4] > 0) & (t[:, 6] > 0) & (t[:, 10] > 0)  # waves that ran the lean loop
    tc = t[ran]
    life = tc[:, 10] - tc[:, 0]
    parts = np.diff(tc, axis=1)
    order = np.argsort(life)
    band = max(len(order) // 100, 1)
    med = order[len(order) // 2 - band: len(order) // 2 + band + 1]
    top = order[int(0.99 * len(order)):]
    res = dict(num_envs=n, waves=int(len(t)), contact_waves=int(ran.sum()), unit='s_memtime ticks')
    for name, sel in (('median_band', med), ('slowest_1pct', top)):
        d = {p: float(parts[sel, k].mean()) for k, p in enumerate(PARTS)}
        lf = float(life[sel].mean())
        res[name] = dict(wave_lifetime=lf, **d, outside_stages=sum(d[p] for p in OUTSIDE),
                         parts_over_lifetime=sum(d.values()) / lf)
    # free waves (no lane in contact): stamps 4..7 absent
    free = (t[:, 4] == 0) & (t[:, 10] > 0) & (t[:, 3] > 0)
    if free.any():
        tf = t[free]
        res['free_waves'] = dict(count=int(free.sum()), wave_lifetime=float((tf[:, 10] - tf[:, 0]).mean()),
                                 prologue_loads=float((tf[:, 1] - tf[:, 0]).mean()),
                                 barrier=float((tf[:, 2] - tf[:, 1]).mean()),
                                 role_frame_flags=float((tf[:, 3] - tf[:, 2]).mean()),
                                 success_reward=float((tf[:, 8] - tf[:, 3]).mean()),
                                 reset_obs=float((tf[:, 9] - tf[:, 8]).mean()),
                                 final_stores=float((tf[:, 10] - tf[:, 9]).mean()))
    # shader clock: the -DOGBX_STAGE_STAMPS=2 build takes an s_memrealtime (100 MHz) beside the first and the last
    # s_memtime stamp (words 11, 12).  Read on the last launch of >= 2 s of back-to-back steps (no synchronize inside).
    import time
    torch.cuda.synchronize()
    _lib.check(L.ogbx_diag_path_stamps(buf))  # clear
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < 2.2:
        for _ in range(256):
            env.step(views[k % 128])
            k += 1
    torch.cuda.synchronize()
    _lib.check(L.ogbx_diag_path_stamps(buf))
    c = np.frombuffer(buf, dtype=np.uint64).reshape(4096, 16)[:nw].astype(np.int64)
    ok = (c[:, 4] > 0) & (c[:, 6] > 0) & (c[:, 10] > 0) & (c[:, 11] > 0) & (c[:, 12] > c[:, 11])
    if ok.any():
        mhz = (c[ok, 10] - c[ok, 0]) / (c[ok, 12] - c[ok, 11]) * 100.0
        res['shader_clock'] = dict(back_to_back_steps=k, contact_waves=int(ok.sum()), median_mhz=float(np.median(mhz)),
                                   p10_mhz=float(np.percentile(mhz, 10)), p90_mhz=float(np.percentile(mhz, 90)),
                                   median_lifetime_ticks=float(np.median(c[ok, 10] - c[ok, 0])),
                                   median_lifetime_realtime_ticks=float(np.median(c[ok, 12] - c[ok, 11])))
    line = json.dumps(res)
    print(line, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], 'w') as f:
            f.write(line + '\n')
    env.close()


if __name__ == '__main__':
    main()
