#!/usr/bin/env python
"""Per-call and per-kernel time of ATC pairs over the episode ring
(GCReplayBuffer.sample_atc) next to the offline ATCDataset over the snapshot.

One ring of N = 1,024 envs and T = 512 slots with 64 x 64 x 6 uint8 frames,
frame_stack 3, p_aug 1, filled with 2 T inserts, twice:

  long     every env done with probability 1/100 per step (episodes near 100
           rows, about five live segments per env), k = 2
  short    episode lengths drawn from 1..3 (c near L: some 256 live segments per
           env, the count kernel's long walk), k = 1

On each, for B = 256 and B = 1,024, the calls alternating in every window:

  table      ogbx_online_atc_table alone (online_atc_count_kernel and the
             scan): the rebuild a sample pays once after every insert or change
             of k
  ring_B     sample_atc(B, k, out=batch) with the table already built: one
             online_atc_sample_kernel launch
  offline_B  ATCDataset(Dataset(snapshot), _periodic=False).sample(B, k,
             out=batch) with valid(k) cached: one atc_sample_kernel launch,
             which composes the same frames

For each: call_us (host clock around windows of --calls calls closed by a
device synchronise), host_us (host time of one call with the device held by a
spin kernel) and kernel_us (launches queued back to back behind a spin kernel
between one HIP event pair), as scripts/probe_online_trl_sampler.py measures
them.

  python scripts/probe_online_atc_sampler.py --out profiles/online_atc_sampler.json
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
N, T, FRAME = 1024, 512, (64, 64, 6)
BATCHES = (256, 1024)
RUNS = {'long': 2, 'short': 1}  # run -> k


def stats(xs):
    s = sorted(xs)
    return dict(values=[round(x, 3) for x in xs], median=round(s[len(s) // 2], 3), min=round(s[0], 3),
                max=round(s[-1], 3))


def fill(torch, buf, run, dev):
    """2 T steps of seeded frames: a full ring that wrapped once."""
    g = torch.Generator(device=dev).manual_seed(7)
    pool = [torch.randint(0, 256, (N,) + FRAME, dtype=torch.uint8, device=dev, generator=g) for _ in range(8)]
    left = torch.randint(1, 4, (N,), device=dev, generator=g)
    for t in range(2 * T):
        if run == 'long':
            done = torch.rand(N, device=dev, generator=g) < 0.01
        else:
            left -= 1
            done = left == 0
            left = torch.where(done, torch.randint(1, 4, (N,), device=dev, generator=g), left)
        buf.add(dict(observations=pool[t % len(pool)]), done)


def measure(args):
    sys.path.insert(0, args.root)
    import torch

    assert torch.cuda.is_available(), 'this probe needs the GPU'
    from ogbench_amd import _lib
    from ogbench_amd.datasets import ATCDataset, Dataset, GCReplayBuffer

    dev = torch.device('cuda', 0)
    raw_stream = torch._C._cuda_getCurrentRawStream

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / args.calls * 1e6

    def host(fn, calls=200):
        torch.cuda.synchronize(dev)
        torch.cuda._sleep(int(calls * 120e-6 * 2.4e9))
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize(dev)
        return dt / calls * 1e6

    def kernel(fn, launches=500):
        stream = torch.cuda.current_stream(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        torch.cuda._sleep(int(launches * 120e-6 * 2.4e9))
        a.record(stream)
        for _ in range(launches):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / launches * 1e3

    buf = GCReplayBuffer.create(dict(observations=torch.zeros(FRAME, dtype=torch.uint8)), N, T, dict(CFG), device=dev,
                                seed=1)
    res = {}
    for run, k in RUNS.items():
        buf.clear()
        fill(torch, buf, run, dev)
        off = ATCDataset(Dataset(buf.snapshot()), dict(CFG), seed=1, _periodic=False)
        fns = {}
        for B in BATCHES:
            rb, ob = buf.sample_atc(B, k), off.sample(B, k)
            fns[f'ring_{B}'] = lambda B=B, b=rb: buf.sample_atc(B, k, out=b)
            fns[f'offline_{B}'] = lambda B=B, b=ob: off.sample(B, k, out=b)

        def table():
            _lib.check(buf._La.ogbx_online_atc_table(buf._ring, k, buf._atc_W.data_ptr(), buf._atc_P.data_ptr(),
                                                     buf._atc_tmp.data_ptr(), buf._atc_tmp.numel(), raw_stream(0)),
                       'online_atc_table')

        fns['table'] = table
        builds = buf.atc_table_builds
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        times = {(name, m): [] for name in fns for m in ('call_us', 'host_us', 'kernel_us')}
        for _ in range(args.reps):  # alternate the calls
            for m, f in (('call_us', window), ('host_us', host), ('kernel_us', kernel)):
                for name, fn in fns.items():
                    times[(name, m)].append(f(fn))
        seq = buf.ep_seq
        first, last = seq[(buf.steps - T) % T].long(), seq[(buf.steps - 1) % T].long()
        calls = {name: {m: stats(times[(name, m)]) for m in ('call_us', 'host_us', 'kernel_us')} for name in fns}
        r = dict(k=k, anchors=int(buf._atc_P[-1]), live_rows=buf.size,
                 mean_live_segments_per_env=round(float((last - first).float().mean()) + 1, 2),
                 table_builds_by_sample_atc=builds, table_temp_bytes=buf._atc_tmp.numel(),
                 bad_samples=buf.atc_bad_samples(), calls=calls)
        for B in BATCHES:
            ring, offl = calls[f'ring_{B}']['kernel_us'], calls[f'offline_{B}']['kernel_us']
            r[f'ring_minus_offline_kernel_us_{B}'] = round(ring['median'] - offl['median'], 3)
            r[f'offline_kernel_spread_us_{B}'] = round(offl['max'] - offl['min'], 3)
        res[run] = r
        del off, fns
        torch.cuda.empty_cache()
    return res, torch.cuda.get_device_name(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=1000, help='calls per timed window')
    ap.add_argument('--reps', type=int, default=5, help='windows per call')
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)  # the tree whose package is measured
    args = ap.parse_args()
    res, device = measure(args)
    rec = dict(
        what='GCReplayBuffer.sample_atc(B, k, out=batch) (online_atc_sample_kernel, table built) next to the table '
             'build alone (ogbx_online_atc_table: online_atc_count_kernel, one wave per env, and the scan) and the '
             'offline ATCDataset.sample over the snapshot (atc_sample_kernel, valid(k) cached); host clock around '
             'windows of calls closed by a device synchronise, host time and back-to-back kernel time behind a spin '
             'kernel',
        device=device, num_envs=N, horizon=T, inserts=2 * T, frame=list(FRAME), frame_stack=CFG['frame_stack'],
        p_aug=CFG['p_aug'], batches=list(BATCHES), calls_per_window=args.calls, host_calls_per_window=200,
        kernel_launches_per_window=500, windows=args.reps, runs=res)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
