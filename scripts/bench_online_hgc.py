#!/usr/bin/env python
"""Per-call time of HGCReplayBuffer.sample(1024) on the GPU.

Shapes (bench_online_replay.py's: synthetic step outputs; rings of 2**22 rows,
filled past their horizon with episodes of about 50 steps):
  pointmaze  N = 65,536 envs, T = 64 slots: observations float64 [2], actions
             float32 [2], next_observations float64 [2], terminals float32
  antmaze    N = 16,384 envs, T = 256 slots, observations float64 [29], actions
             float32 [8]
with the HIQL config of bench.py's hgcsample workload (discount 0.995,
subgoal_steps 100).  Variants, each as a new batch and as an out= refill:

  online     HGCReplayBuffer.sample(1024): one online_hgc_sample_kernel
  hgc_plain  HGCDataset.sample(1024) over a static dataset of the same rows
             (the ring's snapshot), lookahead off -- its refill is the yardstick
  hgc_ahead  the same, lookahead on
  composed   the only composition available before: snapshot() +
             HGCDataset(...) + one sample (a record only; windows of
             --composed-calls)

Windows, alternation, the two call styles and the statistics are
bench_online_replay.py's (bench_visual_sampler.window / stats), three
alternating rounds.  Condition recorded with its numbers:

  hgc_refill_no_slower_than_hgcdataset_plain
      median(online refill) <= median(hgc_plain refill) + spread(hgc_plain refill)
                               + the excess the GC ring showed over its own
                                 yardstick for the same extra dependent round
                                 trip (--gc-record, profiles/online_replay.json:
                                 GCReplayBuffer refill - GCDataset plain refill
                                 at that shape)

  python scripts/bench_online_hgc.py --out profiles/online_hgc.json

--trace-worker runs 200 refills at the pointmaze shape and nothing else (for a
profiler's kernel trace).
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import bench_online_replay as bo  # noqa: E402
import bench_visual_sampler as bv  # noqa: E402

BATCH, SHAPES = bo.BATCH, bo.SHAPES
HIQL = dict(discount=0.995, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3,
            value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0,
            actor_geom_sample=False, gc_negative=True, p_aug=0.0, frame_stack=None, subgoal_steps=100)


def ring_sampler(torch, filled, seed=2):
    """An HGCReplayBuffer of its own over the columns and tables of a filled ring."""
    from ogbench_amd.datasets import HGCReplayBuffer

    b = HGCReplayBuffer(dict(filled), filled.num_envs, filled.horizon, HIQL, device=filled.device, seed=seed)
    b.ep_seq.copy_(filled.ep_seq)
    b.cur_seq.copy_(filled.cur_seq)
    b.ep_end.copy_(filled.ep_end)
    b._steps = b._ring.steps = filled.steps
    return b


def measure_shape(torch, name, args, gc_record):
    from ogbench_amd.datasets import Dataset, HGCDataset

    dev = torch.device('cuda', 0)
    shape = SHAPES[name]
    filled = bo.new_ring(torch, shape, dev)  # no insert touches it below
    snap = filled.snapshot()
    makers = dict(online=lambda: ring_sampler(torch, filled),
                  hgc_plain=lambda: HGCDataset(snap, dict(HIQL, lookahead=False), seed=2),
                  hgc_ahead=lambda: HGCDataset(snap, dict(HIQL, lookahead=True), seed=2))
    fns = {(v, style): f for v, make in makers.items() for style, f in bo.sample_callers(make).items()}
    # at one (seed, call) the ring and the sampler over its snapshot return the same batch
    a, b = makers['online']().sample(BATCH), makers['hgc_plain']().sample(BATCH)
    assert all(torch.equal(a[k], b[k]) for k in a if k != 'terminals')  # the snapshot's also mark the newest rows

    def composed():
        return HGCDataset(Dataset(filled.snapshot()), HIQL, seed=2).sample(BATCH)

    for f in fns.values():
        for _ in range(args.warmup):
            f()
    composed()
    times = {k: [] for k in fns}
    times[('composed', 'new')] = []
    for _ in range(args.reps):  # alternate the variants
        for k, f in fns.items():
            times[k].append(bv.window(torch, f, args.calls))
        times[('composed', 'new')].append(bv.window(torch, composed, args.composed_calls))
    res = {}
    for (v, style), us in times.items():
        res.setdefault(v, {})[style] = bv.stats(us)
    row = sum(v[0].numel() * v.element_size() for v in filled.values())
    ob = filled['observations'][0].numel() * 8
    res_bytes = (row + 10 * ob + 9 * 8) * BATCH  # the buffer's row, ten gathered observation rows, nine scalars
    gc = gc_record['shapes'][name]['variants']['sample']
    excess = round(gc['online']['refill']['median_us'] - gc['gc_plain']['refill']['median_us'], 3)
    yard = res['hgc_plain']['refill']
    mine = res['online']['refill']['median_us']
    bound = round(yard['median_us'] + yard['spread_us'] + excess, 3)
    cond = {'hgc_refill_no_slower_than_hgcdataset_plain': dict(
        online_us=mine, hgc_plain_us=yard['median_us'], spread_hgc_plain_us=yard['spread_us'],
        gc_ring_excess_us=excess, bound_us=bound, hgc_ahead_us=res['hgc_ahead']['refill']['median_us'],
        holds=bool(mine <= bound))}
    return dict(envs=shape['n'], horizon=filled.horizon, observation_dim=shape['ob'], action_dim=shape['act'],
                row_bytes=row, sample_bytes_written=res_bytes, variants=res, conditions=cond)


def trace_worker():
    import torch

    dev = torch.device('cuda', 0)
    ring = ring_sampler(torch, bo.new_ring(torch, SHAPES['pointmaze'], dev))
    batch = ring.sample(BATCH)
    for _ in range(200):
        ring.sample(BATCH, out=batch)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=2000, help='calls per timed window')
    ap.add_argument('--composed-calls', type=int, default=10, help='calls per window of the composed sample')
    ap.add_argument('--reps', type=int, default=3, help='alternating rounds (windows per variant)')
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--gc-record', default=os.path.join(ROOT, 'profiles', 'online_replay.json'),
                    help="the GC ring's record: its excess over its yardstick is the condition's second term")
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--trace-worker', action='store_true', help='only run the kernel at the pointmaze shape')
    args = ap.parse_args()
    if args.trace_worker:
        return trace_worker()
    import torch

    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    with open(args.gc_record) as f:
        gc_record = json.load(f)
    rec = dict(
        what='per-call time of HGCReplayBuffer.sample(1024) against HGCDataset.sample(1024) over a static dataset of '
             'the same rows, host clock around windows of calls closed by a device synchronise',
        device=torch.cuda.get_device_name(0), ring_rows=bo.ROWS, batch=BATCH, calls_per_window=args.calls,
        composed_calls_per_window=args.composed_calls, windows=args.reps, config=HIQL,
        shapes={name: measure_shape(torch, name, args, gc_record) for name in SHAPES})
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
