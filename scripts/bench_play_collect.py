"""Time powderworld play-data collection on one MI355X (profiles/play_collect.json).

  (i)   the plan launch (ogbx_play_plan) at N envs, T steps: device-paced
        windows of back-to-back launches, host clock around a window closed by
        a device synchronise, median over windows;
  (ii)  datagen.collect_powderworld for easy / medium / hard, one round, as
        env-steps/s (host clock around the whole call, closed by a
        synchronise; it includes the env's creation, the reset, the plan, the
        rollouts and the transposing copies), median of the repeats after one
        warm-up call;
  (iii) the rollout-only rate of the same build on the same actions: the same
        chunked rollout loop into a reused [K, N, ...] block, no dataset;
  (iv)  the CPU baseline on one core: tests/play_np.py planning the fixture's
        recorded 1001-step episodes, and the easy NumPy oracle env
        (oracle/powder_np.py) stepping the planned actions; the medium / hard
        oracle is not timed.

Usage: python scripts/bench_play_collect.py [--n 4096] [--t 1001] [--out profiles/play_collect.json]
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--t', type=int, default=1001)
    ap.add_argument('--chunk', type=int, default=48)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--envs', default='easy,medium,hard')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'play_collect.json'))
    a = ap.parse_args()

    import numpy as np
    import torch

    import ogbench_amd
    from ogbench_amd import _play
    from ogbench_amd.datagen import collect_powderworld

    dev = torch.device('cuda', 0)
    N, T = a.n, a.t
    sync = torch.cuda.synchronize
    rec = dict(what='powderworld play-data collection: plan launch, collect_powderworld and rollout-only rates',
               device=torch.cuda.get_device_name(0), num_envs=N, steps=T, chunk=a.chunk, repeats=a.repeats)

    # (i) the plan launch
    kw = dict(size=8, num_elems=5, xy_size=8, p_random_action=0.5, seed=1, device=dev)
    for _ in range(5):
        _play.plan(N, T, **kw)
    sync()
    wins = []
    for w in range(9):
        t0 = time.perf_counter()
        for i in range(20):
            _play.plan(N, T, episode=i, **kw)
        sync()
        wins.append((time.perf_counter() - t0) / 20 * 1e6)
    rec['plan'] = dict(calls_per_window=20, windows_us=[round(x, 2) for x in wins],
                       median_us=round(statistics.median(wins), 2), min_us=round(min(wins), 2),
                       max_us=round(max(wins), 2))

    # (iv) the plan on one CPU core: the NumPy restatement, Philox replaced by a NumPy tape
    import play_np

    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'play_golden.npz'))
    t0 = time.perf_counter()
    for e in range(8):  # the fixture's eight recorded episodes of 1001 steps
        acts_np = play_np.plan_episode(gold['d_tape'][e, :gold['d_tape_len'][e]], 1001, 8, 2, 0.5)[0]
    plan_np_s = (time.perf_counter() - t0) / 8
    from oracle import powder_np

    o = powder_np.Env(32)
    o.reset(np.zeros((32, 32), np.int32), 0, 0, 0)
    t0 = time.perf_counter()
    for t in range(300):
        o.step(int(acts_np[t]))
    step_np_s = (time.perf_counter() - t0) / 300
    rec['cpu_one_core'] = dict(
        what='tests/play_np.py plan of one 1001-step episode; oracle/powder_np.py easy env step (32x32)',
        plan_us_per_episode=round(plan_np_s * 1e6, 1), easy_step_us=round(step_np_s * 1e6, 1),
        easy_env_steps_per_s=round(1.0 / (step_np_s + plan_np_s / 1001)))

    # (ii), (iii)
    rec['envs'] = {}
    for name in a.envs.split(','):
        env_id = f'powderworld-{name}-v0'
        collect_powderworld(env_id, num_envs=N, max_episode_steps=T, seed=0, device=dev, chunk=a.chunk)  # warm-up
        sync()
        times = []
        for r in range(a.repeats):
            t0 = time.perf_counter()
            data = collect_powderworld(env_id, num_envs=N, max_episode_steps=T, seed=r + 1, device=dev, chunk=a.chunk)
            sync()
            times.append(time.perf_counter() - t0)
            del data
        env = ogbench_amd.make(env_id, num_envs=N, device=dev, mode='data_collection', max_episode_steps=T)
        acts = _play.plan(N, T, size=8, num_elems=env._num_elems, xy_size=8, seed=1, device=dev)['actions']
        rtimes = []
        for r in range(a.repeats + 1):
            env.reset(seed=r)
            sync()
            out = None
            t0 = time.perf_counter()
            for s in range(0, T, a.chunk):
                k = min(a.chunk, T - s)
                if out is not None and out['obs'].shape[0] != k:
                    out = None
                out = env.rollout(acts[s:s + k], out=out)
            sync()
            rtimes.append(time.perf_counter() - t0)
        env.close()
        rtimes = rtimes[1:]
        steps = N * T
        c, ro = statistics.median(times), statistics.median(rtimes)
        rec['envs'][name] = dict(
            collect_s=[round(x, 4) for x in times], rollout_only_s=[round(x, 4) for x in rtimes],
            collect_env_steps_per_s=round(steps / c), rollout_only_env_steps_per_s=round(steps / ro),
            collect_over_rollout=round(c / ro, 3), dataset_GB=round(steps * 32 * 32 * 6 / 1e9, 2))
        print(name, rec['envs'][name], flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
