#!/usr/bin/env python
"""Per-call device time of a visual GCReplayBuffer.sample against the only
route there was before it: a ring of pre-stacked frames.

Shapes: uint8 frames 32 x 32 x 6 and 64 x 64 x 6, N = 1,024 envs, T = 64 slots
(65,536 rows), filled past the horizon with episodes of about 50 steps,
sample(256) with the gciql goal config.

  visual     GCReplayBuffer with frame_stack = 3, p_aug = 1 (every call
             crops): online_gc_sample_kernel over the non-image columns, then
             online_visual_gather_kernel over observations, next_observations,
             value_goals and actor_goals; the ring holds unstacked frames
  prestacked GCReplayBuffer without the two keys over [..., 18] frames (what
             inserting FrameStack(env, 3)'s observations gives): the single
             launch of online_gc_sample_kernel, which has no crop

Both are out= refills, timed with device events over windows of --calls calls,
the two variants alternating for --rounds rounds in one process.  The record
holds both rings' bytes, the per-call medians, their ratio per output byte, and
the gather's bytes from shapes (what it reads and writes for one call).

  python scripts/bench_online_visual.py --out profiles/online_visual_ab.txt

--trace-worker SHAPE runs 200 visual samples at one shape and nothing else (for
a profiler's kernel trace).
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, B, F = 1024, 64, 256, 3
SHAPES = {'32x32x6': (32, 32, 6), '64x64x6': (64, 64, 6)}
GCIQL = dict(discount=0.99, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3,
             value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0,
             actor_geom_sample=False, gc_negative=True)


def ring(torch, shape, stacked, dev):
    from ogbench_amd.datasets import GCReplayBuffer

    c = shape[-1] * (F if stacked else 1)
    frame = shape[:-1] + (c,)
    cfg = dict(GCIQL, frame_stack=None if stacked else F, p_aug=None if stacked else 1.0)
    ex = dict(observations=np.zeros(frame, np.uint8), actions=np.zeros(2, np.float32),
              next_observations=np.zeros(frame, np.uint8))
    buf = GCReplayBuffer.create(ex, N, T, cfg, device=dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(2)
    for _ in range(T + 7):  # past the horizon
        rows = dict(observations=torch.randint(0, 256, (N,) + frame, generator=g, device=dev, dtype=torch.uint8),
                    actions=torch.rand(N, 2, generator=g, device=dev),
                    next_observations=torch.randint(0, 256, (N,) + frame, generator=g, device=dev, dtype=torch.uint8))
        buf.add(rows, torch.rand(N, generator=g, device=dev) < 0.02)
    return buf


def ring_bytes(buf):
    return sum(v.numel() * v.element_size() for v in buf.values()) + sum(
        t.numel() * t.element_size() for t in (buf.ep_seq, buf.cur_seq, buf.ep_end))


def window(torch, buf, out, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        buf.sample(B, out=out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # us per call


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--trace-worker', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    np.random.seed(0)
    if args.trace_worker:
        buf = ring(torch, SHAPES[args.trace_worker], False, dev)
        out = buf.sample(B)
        for _ in range(200):
            buf.sample(B, out=out)
        torch.cuda.synchronize()
        return
    lines = [f'visual GCReplayBuffer.sample({B}) against a ring of pre-stacked frames: N = {N}, T = {T}, F = {F}, '
             f'uint8, out= refills, device events, {args.rounds} alternating rounds of {args.calls} calls '
             f'({args.rounds * args.calls} calls per variant after a warm-up window)', '']
    for name, shape in SHAPES.items():
        bufs = {'visual': ring(torch, shape, False, dev), 'prestacked': ring(torch, shape, True, dev)}
        outs = {k: b.sample(B) for k, b in bufs.items()}
        times = {k: [] for k in bufs}
        for k, b in bufs.items():
            window(torch, b, outs[k], args.calls)  # warm-up
        for _ in range(args.rounds):
            for k, b in bufs.items():
                times[k].append(window(torch, b, outs[k], args.calls))
        frame = int(np.prod(shape))
        out_bytes = 4 * B * frame * F  # the four image keys of one batch
        # the gather: F source frames per (sample, key) at most (the XCD's L2 may serve the ones
        # observations and next_observations share), every output byte once
        read_bytes = 4 * B * frame * F
        med = {k: float(np.median(v)) for k, v in times.items()}
        lines += [
            f'shape {name}: frame {frame} B, image keys of one batch {out_bytes} B',
            f'  ring bytes            visual {ring_bytes(bufs["visual"])}  prestacked {ring_bytes(bufs["prestacked"])}'
            f'  (x{ring_bytes(bufs["prestacked"]) / ring_bytes(bufs["visual"]):.2f})',
            *(f'  {k:<10} us per call  median {med[k]:.2f}  windows ' + ' '.join(f'{x:.2f}' for x in times[k])
              for k in bufs),
            f'  ratio visual / prestacked  {med["visual"] / med["prestacked"]:.3f}  (same output bytes; the visual '
            f'path also crops)',
            f'  gather bytes from shapes  read <= {read_bytes}  write {out_bytes}',
            '',
        ]
        del bufs, outs
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
