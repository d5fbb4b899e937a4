#!/usr/bin/env python
"""Per-call time of visual batches (frame stack + random crop) on the GPU.

Synthetic uint8 frames 64 x 64 x 3, 100 equal trajectories of 200 rows (20,000
rows, 246 MB in HBM), batch 256, the gciql goal config.  Variants:

  a      this tree's visual path doing the plain sampler's work: frame_stack=1,
         evaluation=True (no stack, no crop; the same bytes as c)
  b      frame_stack=3, crop on every call (p_aug=1.0)
  hgc_b  HGCDataset, frame_stack=3, crop on every call (a record only)
  c      the plain sampler (frame_stack=None, p_aug=None) of this tree
  copy   device-to-device copy_ of b's image outputs (the bandwidth ceiling)
  parent c measured in a fresh process on another tree (--parent-root: a
         checkout of the parent commit with its libogbx.so built), once before
         and once after the variants above

Each variant is timed in windows of --calls sample() calls closed by a device
synchronise, --reps windows per variant, the variants alternating; both call
styles are timed: ``sample(B)`` (a new batch per call) and
``sample(B, out=batch)`` (refill).  Per variant and style the record holds
every window's per-call time and their median, min, max and spread
(max - min).  The condition recorded as ``a_within_spread_of_c`` is
median(a) - median(c) <= spread(c), against the parent's c when measured.

  python scripts/bench_visual_sampler.py --parent-root /path/to/parent --out profiles/visual_sampler.json
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.environ.get('OGBX_BENCH_ROOT') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GCIQL = dict(discount=0.99, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3,
             value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0,
             actor_geom_sample=False, gc_negative=True)
HIQL = dict(GCIQL, subgoal_steps=25)
N_TRAJ, TRAJ_LEN, BATCH = 100, 200, 256


def dataset(torch, device):
    from ogbench_amd.datasets import Dataset

    R = N_TRAJ * TRAJ_LEN
    g = torch.Generator(device=device).manual_seed(0)
    obs = torch.randint(0, 256, (R, 64, 64, 3), dtype=torch.uint8, device=device, generator=g)
    act = torch.rand((R, 8), device=device, generator=g) * 2 - 1
    term = torch.zeros(R, dtype=torch.float32, device=device)
    term[TRAJ_LEN - 1::TRAJ_LEN] = 1
    return Dataset(dict(observations=obs, actions=act, terminals=term, valids=1.0 - term), device=device)


def window(torch, fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def stats(us):
    s = sorted(us)
    return dict(windows_us=[round(x, 3) for x in us], median_us=round(s[len(s) // 2], 3), min_us=round(s[0], 3),
                max_us=round(s[-1], 3), spread_us=round(s[-1] - s[0], 3))


def callers(make, kw):
    """The two call styles, each on a sampler of its own: a sampler remembers
    only its last two batches for ``out=``, so new batches from the same
    sampler would turn the refill into a new-batch call."""
    new, refill = make(), make()
    batch = refill.sample(BATCH, **kw)
    return {'new': lambda: new.sample(BATCH, **kw), 'refill': lambda: refill.sample(BATCH, out=batch, **kw)}


def measure(variants, torch, calls, reps, warmup):
    fns = {(v, style): f for v, (make, kw) in variants.items() for style, f in callers(make, kw).items()}
    for f in fns.values():
        for _ in range(warmup):
            f()
    times = {k: [] for k in fns}
    for _ in range(reps):  # alternate the variants
        for k, f in fns.items():
            times[k].append(window(torch, f, calls))
    return {v: {style: stats(times[(v, style)]) for style in ('new', 'refill')} for v in variants}


def plain_worker(args):
    import torch

    from ogbench_amd.datasets import GCDataset

    ds = dataset(torch, 'cuda:0')
    make = lambda: GCDataset(ds, dict(GCIQL, frame_stack=None, p_aug=None), seed=1)  # noqa: E731
    print('RESULT ' + json.dumps(measure({'c': (make, {})}, torch, args.calls, args.reps, args.warmup)['c']))


def run_parent(root, args):
    env = dict(os.environ, OGBX_BENCH_ROOT=root)
    env.pop('OGBX_LIB', None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--plain-worker', '--calls', str(args.calls),
                        '--reps', str(args.reps), '--warmup', str(args.warmup)], cwd=root, env=env,
                       capture_output=True, text=True, timeout=args.step_timeout)
    if p.returncode != 0:
        raise RuntimeError(f'parent worker failed ({p.returncode}):\n{p.stdout}\n{p.stderr}')
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=2000, help='sample() calls per timed window')
    ap.add_argument('--reps', type=int, default=9, help='windows per variant')
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--parent-root', default=None, help="a built checkout of the parent commit (variant 'parent')")
    ap.add_argument('--step-timeout', type=int, default=240, help='time limit of a parent worker, seconds')
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--plain-worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.plain_worker:
        return plain_worker(args)

    parent = [run_parent(args.parent_root, args)] if args.parent_root else []

    import torch

    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    from ogbench_amd.datasets import GCDataset, HGCDataset

    ds = dataset(torch, 'cuda:0')
    variants = {
        'a': (lambda: GCDataset(ds, dict(GCIQL, frame_stack=1, p_aug=None), seed=1), dict(evaluation=True)),
        'b': (lambda: GCDataset(ds, dict(GCIQL, frame_stack=3, p_aug=1.0), seed=1), {}),
        'hgc_b': (lambda: HGCDataset(ds, dict(HIQL, frame_stack=3, p_aug=1.0), seed=1), {}),
        'c': (lambda: GCDataset(ds, dict(GCIQL, frame_stack=None, p_aug=None), seed=1), {}),
    }
    res = measure(variants, torch, args.calls, args.reps, args.warmup)

    # the ceiling: a device-to-device copy of b's image outputs
    b = variants['b'][0]().sample(BATCH)
    images = [b[k] for k in ('observations', 'next_observations', 'value_goals', 'actor_goals')]
    dsts = [torch.empty_like(t) for t in images]

    def copy():
        for d, s in zip(dsts, images):
            d.copy_(s)

    for _ in range(args.warmup):
        copy()
    res['copy'] = stats([window(torch, copy, args.calls) for _ in range(args.reps)])
    b_bytes = sum(t.numel() * t.element_size() for t in images)
    res['copy']['bytes'] = b_bytes
    res['copy']['GB_per_s_written'] = round(b_bytes / res['copy']['median_us'] / 1e3, 1)
    for style in ('new', 'refill'):
        res['b'][style]['GB_per_s_written'] = round(b_bytes / res['b'][style]['median_us'] / 1e3, 1)

    if args.parent_root:
        parent.append(run_parent(args.parent_root, args))
        res['parent'] = {style: stats([x for run in parent for x in run[style]['windows_us']])
                         for style in ('new', 'refill')}
    ref = res.get('parent', res['c'])
    gate = {style: dict(a_minus_c_us=round(res['a'][style]['median_us'] - ref[style]['median_us'], 3),
                        spread_c_us=ref[style]['spread_us'],
                        a_within_spread_of_c=bool(res['a'][style]['median_us'] - ref[style]['median_us']
                                                  <= ref[style]['spread_us']))
            for style in ('new', 'refill')}
    rec = dict(
        what='per-call time of GCDataset/HGCDataset.sample on visual data, host clock around windows of calls '
             'closed by a device synchronise',
        device=torch.cuda.get_device_name(0), rows=N_TRAJ * TRAJ_LEN, frame=[64, 64, 3], batch=BATCH,
        calls_per_window=args.calls, windows=args.reps, c_reference='parent' if args.parent_root else 'this tree',
        variants=res, condition=gate)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
