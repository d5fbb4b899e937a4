#!/usr/bin/env python
"""Per-call time of a NEW ATC batch (no out=): GCReplayBuffer.sample_atc(B, k)
and ATCDataset.sample(B, k) over the ring's snapshot (the table path).

One ring of N = 1,024 envs and T = 64 slots with 64 x 64 x 6 uint8 frames,
frame_stack 3, p_aug 1, filled with 2 T inserts, every env done with
probability 1/20 per step; B = 256, k = 2.  The two calls alternate; each
window is --calls calls closed by a device synchronise, host clock.  The rows
scripts/probe_online_atc_sampler.py does not have (it measures out= refills).

  python scripts/bench_atc_new_batch.py --out new_batch.json [--root TREE]
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(discount=0.99, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3, value_geom_sample=True,
           actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0, actor_geom_sample=False,
           gc_negative=True, p_aug=1.0, frame_stack=3)
N, T, FRAME, B, K = 1024, 64, (64, 64, 6), 256, 2


def stats(xs):
    s = sorted(xs)
    return dict(values=[round(x, 3) for x in xs], median=round(s[len(s) // 2], 3), min=round(s[0], 3),
                max=round(s[-1], 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=500, help='calls per timed window')
    ap.add_argument('--reps', type=int, default=7, help='windows per call')
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--root', default=ROOT, help='the built tree whose package is measured')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    from ogbench_amd.datasets import ATCDataset, Dataset, GCReplayBuffer

    dev = torch.device('cuda', 0)
    buf = GCReplayBuffer.create(dict(observations=torch.zeros(FRAME, dtype=torch.uint8)), N, T, dict(CFG), device=dev,
                                seed=1)
    g = torch.Generator(device=dev).manual_seed(7)
    pool = [torch.randint(0, 256, (N,) + FRAME, dtype=torch.uint8, device=dev, generator=g) for _ in range(8)]
    for t in range(2 * T):
        buf.add(dict(observations=pool[t % len(pool)]), torch.rand(N, device=dev, generator=g) < 0.05)
    off = ATCDataset(Dataset(buf.snapshot()), dict(CFG), seed=1, _periodic=False)
    fns = {'ring_new': lambda: buf.sample_atc(B, K), 'offline_new': lambda: off.sample(B, K)}

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / args.calls * 1e6

    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    times = {name: [] for name in fns}
    for _ in range(args.reps):
        for name, fn in fns.items():
            times[name].append(window(fn))
    res = dict(device=torch.cuda.get_device_name(0), N=N, T=T, frame=FRAME, B=B, k=K, calls=args.calls,
               new_batch={name: dict(call_us=stats(v)) for name, v in times.items()})
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
