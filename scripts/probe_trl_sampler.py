#!/usr/bin/env python
"""Per-call and per-kernel time of TRL batches of GCDataset next to the plain
GC sampler, and the GC / HGC benchmark of this tree next to the parent's.

Layout: a pointmaze-like buffer, observations 2 x f32, actions 2 x f32, 1,000
equal trajectories of 1,000 rows (1 M rows), batch 1024, the crl sampling
probabilities with geometric value goals.  Two samplers over it:

  trl  agent_name='trl': one trl_sample_kernel launch per call (direct path)
  gc   the same config without the agent name, lookahead=False: one
       gc_sample_kernel launch per call

For each, with ``sample(1024, out=batch)`` (refill, no per-call allocation):

  call_us       host clock around windows of --calls calls closed by a device
                synchronise, --reps windows, the two samplers alternating
  host_us       host time of one call over 200 calls with the device held by a
                spin kernel (no call waits on the GPU, and the launches fit the
                queue): Python + ctypes + checks + launch
  kernel_us     1,000 launches queued back to back behind a spin kernel between
                one HIP event pair on the launch stream, per launch
  gathered_bytes  distinct (source, selector) row bytes written per call, and
                scalar_bytes for the per-sample scalar outputs

--parent-root DIR (a built checkout of the parent commit): also runs the
unchanged ``bench.py --workload gcsample`` and ``--workload hgcsample`` three
times each in DIR and in this tree, alternating, each in a fresh process, and
records every value; ``within_parent_spread`` says whether this tree's median
lies inside the parent's own min..max, ``this_median_not_below_parent_min``
whether it is at least the parent's slowest run.

  python scripts/probe_trl_sampler.py --parent-root /path/to/parent --out profiles/trl_sampler.json
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(discount=0.99, value_p_curgoal=0.0, value_p_trajgoal=1.0, value_p_randomgoal=0.0, value_geom_sample=True,
           actor_p_curgoal=0.0, actor_p_trajgoal=0.5, actor_p_randomgoal=0.5, actor_geom_sample=False,
           gc_negative=False, p_aug=None, frame_stack=None)
N_TRAJ, TRAJ_LEN, BATCH = 1000, 1000, 1024


def stats(xs):
    s = sorted(xs)
    return dict(values=[round(x, 3) for x in xs], median=round(s[len(s) // 2], 3), min=round(s[0], 3),
                max=round(s[-1], 3))


def run_bench(root, workload, steps, warmup, limit):
    env = dict(os.environ)
    env.pop('OGBX_LIB', None)
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--workload', workload], cwd=root, env=env, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise RuntimeError(f'bench.py {workload} in {root} failed ({p.returncode}):\n{p.stdout}\n{p.stderr}')
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1]
    r = json.loads(line)
    return dict(value=r['value'], ms_per_step=r['ms_per_step'], kernel_ms=r['roofline']['kernel_ms'])


def parent_comparison(args):
    out = {}
    for workload in ('gcsample', 'hgcsample'):
        runs = {'parent': [], 'this': []}
        for _ in range(3):  # alternate the trees
            for name, root in (('parent', args.parent_root), ('this', ROOT)):
                runs[name].append(run_bench(root, workload, args.bench_steps, args.bench_warmup, args.step_timeout))
        rec = {name: dict(samples_per_s=stats([r['value'] for r in rs]),
                          us_per_step=stats([r['ms_per_step'] * 1e3 for r in rs]),
                          kernel_us=stats([r['kernel_ms'] * 1e3 for r in rs])) for name, rs in runs.items()}
        p, t = rec['parent']['samples_per_s'], rec['this']['samples_per_s']
        rec['within_parent_spread'] = bool(p['min'] <= t['median'] <= p['max'])
        rec['this_median_not_below_parent_min'] = bool(t['median'] >= p['min'])
        rec['this_median_over_parent_median'] = round(t['median'] / p['median'], 4)
        out[workload] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=5000, help='sample() calls per timed window')
    ap.add_argument('--reps', type=int, default=9, help='windows per sampler')
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--parent-root', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--bench-steps', type=int, default=50000)
    ap.add_argument('--bench-warmup', type=int, default=1000)
    ap.add_argument('--step-timeout', type=int, default=240, help='time limit of one bench.py run, seconds')
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    args = ap.parse_args()

    # fresh processes first, before this one opens the GPU
    bench = parent_comparison(args) if args.parent_root else None

    import torch

    assert torch.cuda.is_available(), 'this probe needs the GPU'
    from ogbench_amd.datasets import Dataset, GCDataset

    dev = torch.device('cuda', 0)
    R = N_TRAJ * TRAJ_LEN
    g = torch.Generator(device=dev).manual_seed(0)
    term = torch.zeros(R, dtype=torch.float32, device=dev)
    term[TRAJ_LEN - 1::TRAJ_LEN] = 1
    ds = Dataset(dict(observations=torch.randn(R, 2, device=dev, generator=g),
                      actions=torch.rand(R, 2, device=dev, generator=g) * 2 - 1, terminals=term,
                      valids=1.0 - term), device=dev)
    samplers = {'trl': GCDataset(ds, dict(CFG, agent_name='trl'), seed=1),
                'gc': GCDataset(ds, dict(CFG, lookahead=False), seed=1)}
    batches = {k: s.sample(BATCH) for k, s in samplers.items()}
    fns = {k: (lambda s=s, b=batches[k]: s.sample(BATCH, out=b)) for k, s in samplers.items()}

    # trl_gc_columns: ogbx_trl_sample over the GC sampler's seven columns alone
    # (selectors 0..3) -- the midpoint draw, its selector and the two offset
    # outputs without the midpoint's columns
    import ctypes

    from ogbench_amd import _lib
    from ogbench_amd import datasets as D

    t = samplers['trl']
    select = {'next_observations': ('observations', 1), 'value_goals': ('observations', 2),
              'actor_goals': ('observations', 3)}
    lean = {k: torch.empty_like(v) for k, v in batches['gc'].items()}
    lean.update(value_offsets=torch.empty(BATCH, dtype=torch.int64, device=dev),
                value_midpoint_offsets=torch.empty(BATCH, dtype=torch.int64, device=dev))
    cols = [t._column(*select.get(k, (k, 0))[:1], lean[k], select.get(k, (k, 0))[1])
            for k in batches['gc'] if k not in ('masks', 'rewards')]
    col_arr = (D.GcColumn * len(cols))(*cols)
    col_ptr = ctypes.cast(col_arr, ctypes.c_void_p)
    outs = D.TrlOutputs(None, None, None, None, lean['value_offsets'].data_ptr(),
                        lean['value_midpoint_offsets'].data_ptr(), lean['masks'].data_ptr(),
                        lean['rewards'].data_ptr(), None)
    raw_stream = torch._C._cuda_getCurrentRawStream
    calls = [0]

    def trl_gc_columns():
        calls[0] += 1
        _lib.check(t._L.ogbx_trl_sample(t._buf, t._cfg, col_ptr, len(cols), BATCH, 1, None, None, 1, calls[0], outs,
                                        None, None, raw_stream(0)), 'trl_sample')

    batches['trl_gc_columns'] = lean
    fns['trl_gc_columns'] = trl_gc_columns

    def window(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / args.calls * 1e6

    def host(fn, calls=200):
        # few enough launches to fit the queue behind the spin kernel: with
        # thousands the host ends up waiting for the spin kernel itself
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

    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    times = {(k, m): [] for k in fns for m in ('call_us', 'host_us', 'kernel_us')}
    for _ in range(args.reps):  # alternate the samplers
        for m, f in (('call_us', window), ('host_us', host), ('kernel_us', kernel)):
            for k, fn in fns.items():
                times[(k, m)].append(f(fn))
    res = {}
    for k, batch in batches.items():
        seen, gathered, scalar = set(), 0, 0
        for name, t in batch.items():
            if t.data_ptr() in seen:
                continue
            seen.add(t.data_ptr())
            nbytes = t.numel() * t.element_size()
            if name in ('masks', 'rewards', 'value_offsets', 'value_midpoint_offsets'):
                scalar += nbytes
            else:
                gathered += nbytes
        res[k] = dict(keys=len(batch), distinct_tensors=len(seen), gathered_bytes=gathered, scalar_bytes=scalar,
                      **{m: stats(times[(k, m)]) for m in ('call_us', 'host_us', 'kernel_us')})
    ratio = {m: round(res['trl'][m]['median'] / res['gc'][m]['median'], 3) for m in ('call_us', 'host_us', 'kernel_us')}
    ratio['gathered_bytes'] = round(res['trl']['gathered_bytes'] / res['gc']['gathered_bytes'], 3)
    rec = dict(
        what='GCDataset.sample(1024, out=batch) with a TRL agent name (trl_sample_kernel) next to the plain GC '
             'sampler with lookahead=False (gc_sample_kernel); host clock around windows of calls closed by a '
             'device synchronise, host time and back-to-back kernel time behind a spin kernel; trl_gc_columns: ogbx_trl_sample called directly over the GC sampler\'s seven columns alone',
        device=torch.cuda.get_device_name(0), rows=R, observation_bytes=8, action_bytes=8, batch=BATCH,
        calls_per_window=args.calls, host_calls_per_window=200, kernel_launches_per_window=1000,
        windows=args.reps, samplers=res, trl_over_gc=ratio,
        parent_comparison=bench,
        parent_comparison_method=None if bench is None else
        f'bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} --workload W, three fresh '
        f'processes per tree, the trees alternating')
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
