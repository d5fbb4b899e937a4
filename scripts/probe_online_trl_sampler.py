#!/usr/bin/env python
"""Per-call and per-kernel time of TRL batches over the episode ring next to
the non-TRL ring sampler and the offline TRL sampler over the snapshot.

Two full rings, batch 1024, observations 2 x f32, actions 2 x f32, an own
next_observations column, the crl sampling probabilities with geometric value
goals, every env done with probability 1/100 per step:

  n1024_t1000    N = 1,024 envs,  T = 1,000 steps (about ten live closed
                 episodes per env: the ordinal search has something to do)
  n65536_t16     N = 65,536 envs, T = 16 steps (the env search is 16 levels)

On each ring, the calls alternating in every window:

  trl        GCReplayBuffer with agent_name='trl', sample(1024, out=batch) with
             the table already built for this step: one
             online_trl_sample_kernel launch
  table      ogbx_online_trl_table alone: the rebuild a sample pays once after
             every insert
  gc_ring    the same ring without the agent name, sample(1024, out=batch): one
             online_gc_sample_kernel launch.  With --parent-root DIR (a built
             checkout of the parent commit) this entry is also measured by a
             fresh process running in DIR, as ``gc_ring_parent``
  offline    GCDataset(Dataset(ring.snapshot()), agent_name='trl'),
             sample(1024, out=batch): one trl_sample_kernel launch over the
             compacted pick table

For each: call_us (host clock around windows of --calls calls closed by a
device synchronise), host_us (host time of one call with the device held by a
spin kernel) and kernel_us (launches queued back to back behind a spin kernel
between one HIP event pair), as scripts/probe_trl_sampler.py measures them.

  python scripts/probe_online_trl_sampler.py --parent-root /path/to/parent --out profiles/online_trl_sampler.json
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = dict(discount=0.99, value_p_curgoal=0.0, value_p_trajgoal=1.0, value_p_randomgoal=0.0, value_geom_sample=True,
           actor_p_curgoal=0.0, actor_p_trajgoal=0.5, actor_p_randomgoal=0.5, actor_geom_sample=False,
           gc_negative=False, p_aug=None, frame_stack=None)
SHAPES = {'n1024_t1000': (1024, 1000), 'n65536_t16': (65536, 16)}
BATCH, P_DONE = 1024, 0.01


def stats(xs):
    s = sorted(xs)
    return dict(values=[round(x, 3) for x in xs], median=round(s[len(s) // 2], 3), min=round(s[0], 3),
                max=round(s[-1], 3))


def fill(torch, bufs, N, T, dev):
    """T + 3 steps of seeded rows into every buffer: a full ring that wrapped."""
    g = torch.Generator(device=dev).manual_seed(N + T)
    for _ in range(T + 3):
        rows = dict(observations=torch.randn(N, 2, device=dev, generator=g),
                    actions=torch.rand(N, 2, device=dev, generator=g) * 2 - 1,
                    next_observations=torch.randn(N, 2, device=dev, generator=g))
        done = torch.rand(N, device=dev, generator=g) < P_DONE
        for b in bufs:
            b.add(rows, done)


def measure(args, only_gc):
    sys.path.insert(0, args.root)
    import torch

    assert torch.cuda.is_available(), 'this probe needs the GPU'
    from ogbench_amd.datasets import Dataset, GCDataset, GCReplayBuffer

    dev = torch.device('cuda', 0)
    ex = dict(observations=torch.zeros(2), actions=torch.zeros(2), next_observations=torch.zeros(2))

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / args.calls * 1e6

    def host(fn, calls=200):
        torch.cuda.synchronize(dev)
        torch.cuda._sleep(int(calls * 60e-6 * 2.4e9))
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize(dev)
        return dt / calls * 1e6

    def kernel(fn, launches=1000):
        stream = torch.cuda.current_stream(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        torch.cuda._sleep(int(launches * 60e-6 * 2.4e9))
        a.record(stream)
        for _ in range(launches):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / launches * 1e3

    res = {}
    for shape, (N, T) in SHAPES.items():
        gc = GCReplayBuffer.create(ex, N, T, dict(CFG), device=dev, seed=1)
        bufs = [gc]
        if not only_gc:
            trl = GCReplayBuffer.create(ex, N, T, dict(CFG, agent_name='trl'), device=dev, seed=1)
            bufs.append(trl)
        fill(torch, bufs, N, T, dev)
        batches = {'gc_ring': gc.sample(BATCH)}
        fns = {'gc_ring': lambda b=batches['gc_ring']: gc.sample(BATCH, out=b)}
        extra = {}
        if not only_gc:
            from ogbench_amd import _lib

            off = GCDataset(Dataset(trl.snapshot()), dict(CFG, agent_name='trl'), seed=1)
            batches['trl'] = trl.sample(BATCH)
            batches['offline'] = off.sample(BATCH)
            fns['trl'] = lambda b=batches['trl']: trl.sample(BATCH, out=b)
            fns['offline'] = lambda b=batches['offline']: off.sample(BATCH, out=b)
            raw_stream = torch._C._cuda_getCurrentRawStream

            def table():
                _lib.check(trl._Lt.ogbx_online_trl_table(trl._ring, trl._trl_P.data_ptr(), trl._trl_tmp.data_ptr(),
                                                         trl._trl_tmp.numel(), raw_stream(0)), 'online_trl_table')

            fns['table'] = table
            extra = dict(pickable_rows=int(trl._trl_P[-1]), live_rows=trl.size, table_builds=trl.trl_table_builds,
                         table_temp_bytes=trl._trl_tmp.numel(), bad_samples=trl.trl_bad_samples())
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        times = {(k, m): [] for k in fns for m in ('call_us', 'host_us', 'kernel_us')}
        for _ in range(args.reps):  # alternate the calls
            for m, f in (('call_us', window), ('host_us', host), ('kernel_us', kernel)):
                for k, fn in fns.items():
                    times[(k, m)].append(f(fn))
        res[shape] = dict(num_envs=N, horizon=T, **extra,
                          calls={k: {m: stats(times[(k, m)]) for m in ('call_us', 'host_us', 'kernel_us')}
                                 for k in fns})
        del bufs, fns, batches
    return res, torch.cuda.get_device_name(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=5000, help='calls per timed window')
    ap.add_argument('--reps', type=int, default=7, help='windows per call')
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--parent-root', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--step-timeout', type=int, default=300, help='time limit of the parent process, seconds')
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)  # the tree whose package is measured
    ap.add_argument('--only-gc', action='store_true', help=argparse.SUPPRESS)  # the parent's part, printed as JSON
    args = ap.parse_args()

    if args.only_gc:
        res, _ = measure(args, True)
        print('RESULT ' + json.dumps(res))
        return

    parent = None
    if args.parent_root:  # a fresh process first, before this one opens the GPU
        args.parent_root = os.path.abspath(args.parent_root)
        env = dict(os.environ)
        env.pop('OGBX_LIB', None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--only-gc', '--root', args.parent_root,
                            '--calls', str(args.calls), '--reps', str(args.reps), '--warmup', str(args.warmup)],
                           cwd=args.parent_root, env=env, capture_output=True, text=True, timeout=args.step_timeout)
        if p.returncode != 0:
            raise RuntimeError(f'the parent process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}')
        parent = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])

    res, device = measure(args, False)
    for shape, r in res.items():
        c = r['calls']
        if parent is not None:
            c['gc_ring_parent'] = parent[shape]['calls']['gc_ring']
        r['trl_over_gc_ring'] = {m: round(c['trl'][m]['median'] / c['gc_ring'][m]['median'], 3)
                                 for m in ('call_us', 'host_us', 'kernel_us')}
        r['trl_minus_gc_ring_kernel_us'] = round(c['trl']['kernel_us']['median'] - c['gc_ring']['kernel_us']['median'], 3)
        r['trl_over_offline'] = {m: round(c['trl'][m]['median'] / c['offline'][m]['median'], 3)
                                 for m in ('call_us', 'host_us', 'kernel_us')}
    rec = dict(
        what='GCReplayBuffer.sample(1024, out=batch) with a TRL agent name (online_trl_sample_kernel, table built) '
             'next to the table rebuild alone (ogbx_online_trl_table), the non-TRL ring sampler '
             '(online_gc_sample_kernel; gc_ring_parent: the same call by a fresh process in a checkout of the parent '
             'commit) and the offline TRL sampler over the snapshot (trl_sample_kernel); host clock around windows '
             'of calls closed by a device synchronise, host time and back-to-back kernel time behind a spin kernel',
        device=device, batch=BATCH, done_probability=P_DONE, observation_bytes=8, action_bytes=8,
        calls_per_window=args.calls, host_calls_per_window=200, kernel_launches_per_window=1000, windows=args.reps,
        rings=res)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
