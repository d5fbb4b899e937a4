#!/usr/bin/env python
"""Per-call time of ATC batches (anchor / positive pairs) on the GPU.

Synthetic uint8 frames 64 x 64 x 3, 100 equal trajectories of 200 rows (20,000
rows, 246 MB in HBM; the dataset of bench_visual_sampler.py), batch 256,
frame_stack 3, crop on every call (p_aug 1.0, padding 4), k = 3.  Variants:

  atc       ATCDataset.sample(256, 3): one atc_sample_kernel launch
  composed  the same batch from what the library offered before ogbx_atc.h:
            torch.randint into a prebuilt valid(3), idx + k, and one
            ogbx_visual_gather with two columns (selector 0 through idxs,
            selector 2 through value_goal_idxs = idx + k; padding 4, draw_crop 1)
  copy      device-to-device copy_ of the two outputs (the bandwidth ceiling)
  vis_b     GCDataset with frame_stack 3 and crop (variant b of
            bench_visual_sampler.py) on this tree and, in a fresh process, on
            --parent-root (a checkout of the parent commit with its libogbx.so
            built), once before and once after the variants above

Windows, repetitions, alternation, the two call styles and the statistics are
bench_visual_sampler.py's.  Conditions recorded, each against the yardstick's
own spread:

  atc_within_spread_of_composed   median(atc) <= median(composed) + spread(composed)
  vis_b_within_spread_of_parent   median(vis_b here) - median(vis_b parent) <= spread(vis_b parent)

  python scripts/bench_atc_sampler.py --parent-root /path/to/parent --out profiles/atc_sampler.json
"""

import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.environ.get('OGBX_BENCH_ROOT') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import bench_visual_sampler as bv  # noqa: E402  (sys.path[0] is ROOT, so it imports that tree's package)

BATCH, K, STACK, PADDING = bv.BATCH, 3, 3, 4
ATC_CFG = dict(frame_stack=STACK, p_aug=1.0, augment_padding=PADDING)
VIS_B_CFG = dict(bv.GCIQL, frame_stack=STACK, p_aug=1.0)
STYLES = ('new', 'refill')


class Composed:
    """The ATC batch from randint + one two-column ogbx_visual_gather, with
    the call styles of a sampler (``sample(B)`` / ``sample(B, out=batch)``)."""

    def __init__(self, torch, ds, seed=1):
        from ogbench_amd import _lib
        from ogbench_amd import datasets as D

        self.torch, self._lib, self.D = torch, _lib, D
        self.src = ds['observations']
        helper = D.ATCDataset(ds, dict(ATC_CFG), seed=seed, _periodic=False)  # the tables only
        self.table, self.n = helper._valid_k(K)
        self.buf, self.keep = helper._buf, helper
        self.L = D._bind()
        self.seed, self.calls = seed, 0
        self.cols = {}

    def batch(self, B):
        torch, D, src = self.torch, self.D, self.src
        H, W, C = src.shape[1:]
        out = {k: torch.empty((B, H, W, C * STACK), dtype=src.dtype, device=src.device)
               for k in ('observations', 'positive_observations')}
        cols = (D.VisualColumn * 2)(
            D.VisualColumn(src.data_ptr(), out['observations'].data_ptr(), H, W, C, 0, 1, 1),
            D.VisualColumn(src.data_ptr(), out['positive_observations'].data_ptr(), H, W, C, 2, 1, 1))
        self.cols = {id(out): (out, cols)}
        return out, cols

    def sample(self, B, out=None):
        torch, lib = self.torch, self._lib
        hit = self.cols.get(id(out)) if out is not None else None
        out, cols = hit if hit is not None else self.batch(B)
        idx = self.table[torch.randint(self.n, (B,), device=self.src.device)]
        pos = idx + K
        vidx = self.D.VisualIndices(idx.data_ptr(), pos.data_ptr(), None, None)
        call, self.calls = self.calls, self.calls + 1
        lib.check(self.L.ogbx_visual_gather(self.buf, None, ctypes.cast(cols, ctypes.c_void_p), 2, B, vidx, STACK,
                                            PADDING, None, 1, self.seed, call, None,
                                            lib.stream_of(self.src.device)), 'visual_gather')
        return out


def vis_b_worker(args):
    import torch

    from ogbench_amd.datasets import GCDataset

    ds = bv.dataset(torch, 'cuda:0')
    make = lambda: GCDataset(ds, dict(VIS_B_CFG), seed=1)  # noqa: E731
    res = bv.measure({'vis_b': (make, {})}, torch, args.calls, args.reps, args.warmup)['vis_b']
    print('RESULT ' + json.dumps(res))


def run_parent(root, args):
    env = dict(os.environ, OGBX_BENCH_ROOT=root)
    env.pop('OGBX_LIB', None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--vis-b-worker', '--calls', str(args.calls),
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
    ap.add_argument('--parent-root', default=None, help='a built checkout of the parent commit (vis_b there)')
    ap.add_argument('--step-timeout', type=int, default=240, help='time limit of a parent worker, seconds')
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--vis-b-worker', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.vis_b_worker:
        return vis_b_worker(args)

    parent = [run_parent(args.parent_root, args)] if args.parent_root else []

    import torch

    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    from ogbench_amd.datasets import ATCDataset, GCDataset

    ds = bv.dataset(torch, 'cuda:0')
    variants = {
        'atc': (lambda: ATCDataset(ds, dict(ATC_CFG), seed=1), dict(k=K)),
        'composed': (lambda: Composed(torch, ds), {}),
        'vis_b': (lambda: GCDataset(ds, dict(VIS_B_CFG), seed=1), {}),
    }
    # the two batches agree in shape and dtype (their draws differ: Philox pick against torch.randint)
    a, c = variants['atc'][0]().sample(BATCH, k=K), variants['composed'][0]().sample(BATCH)
    assert list(a) == list(c) and all(a[k].shape == c[k].shape and a[k].dtype == c[k].dtype for k in a)
    res = bv.measure(variants, torch, args.calls, args.reps, args.warmup)

    # the ceiling: a device-to-device copy of the two outputs
    images = list(a.values())
    dsts = [torch.empty_like(t) for t in images]

    def copy():
        for d, s in zip(dsts, images):
            d.copy_(s)

    for _ in range(args.warmup):
        copy()
    res['copy'] = bv.stats([bv.window(torch, copy, args.calls) for _ in range(args.reps)])
    nbytes = sum(t.numel() * t.element_size() for t in images)
    res['copy']['bytes'] = nbytes
    res['copy']['GB_per_s_written'] = round(nbytes / res['copy']['median_us'] / 1e3, 1)
    for v in ('atc', 'composed'):
        for style in STYLES:
            res[v][style]['GB_per_s_written'] = round(nbytes / res[v][style]['median_us'] / 1e3, 1)

    cond = {'atc_within_spread_of_composed': {
        style: dict(atc_minus_composed_us=round(res['atc'][style]['median_us'] - res['composed'][style]['median_us'], 3),
                    spread_composed_us=res['composed'][style]['spread_us'],
                    holds=bool(res['atc'][style]['median_us']
                               <= res['composed'][style]['median_us'] + res['composed'][style]['spread_us']))
        for style in STYLES}}
    if args.parent_root:
        parent.append(run_parent(args.parent_root, args))
        res['vis_b_parent'] = {style: bv.stats([x for run in parent for x in run[style]['windows_us']])
                               for style in STYLES}
        cond['vis_b_within_spread_of_parent'] = {
            style: dict(here_minus_parent_us=round(res['vis_b'][style]['median_us']
                                                   - res['vis_b_parent'][style]['median_us'], 3),
                        spread_parent_us=res['vis_b_parent'][style]['spread_us'],
                        holds=bool(res['vis_b'][style]['median_us'] - res['vis_b_parent'][style]['median_us']
                                   <= res['vis_b_parent'][style]['spread_us']))
            for style in STYLES}
    rec = dict(
        what='per-call time of ATCDataset.sample and of the same batch composed from randint + ogbx_visual_gather, '
             'host clock around windows of calls closed by a device synchronise',
        device=torch.cuda.get_device_name(0), rows=bv.N_TRAJ * bv.TRAJ_LEN, frame=[64, 64, 3], batch=BATCH,
        frame_stack=STACK, padding=PADDING, k=K, calls_per_window=args.calls, windows=args.reps,
        parent_measured=bool(args.parent_root), variants=res, conditions=cond)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
