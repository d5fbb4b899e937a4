#!/usr/bin/env python
"""Per-call time of GCReplayBuffer inserts and hindsight samples on the GPU.

Shapes (synthetic step outputs; rings of 2**22 rows, filled past their horizon
with episodes of about 50 steps):
  pointmaze  N = 65,536 envs, T = 64 slots: observations float64 [2], actions
             float32 [2], next_observations float64 [2] taken from
             final_observation where done (15 % of the envs), terminals float32
  antmaze    N = 16,384 envs, T = 256 slots, observations float64 [29], actions
             float32 [8]
and sample(1024) on each, with the gciql goal config.  Variants:

  insert   online        GCReplayBuffer.add_step(terminated, truncated): the
                         elementwise terminated | truncated and one
                         online_insert_kernel launch
           online_done   GCReplayBuffer.add_step(done, None): the launch alone
           replay        ReplayBuffer.add_step on the SAC layout (existing
                         code: observations, actions, rewards, masks,
                         next_observations; 56 / 512 B per row against the
                         ring's 44 / 500 B + 4 B of ep_seq) -- the yardstick
           replay_same   ReplayBuffer.add_transitions on the ring's own four
                         columns (no final_observation: it has no alt there)
  sample   online        GCReplayBuffer.sample(1024), new batch / out= refill
           gc_ahead      GCDataset.sample(1024) over a static dataset of the
           gc_plain      same rows (the ring's snapshot), lookahead on / off
                         -- gc_plain's refill is the yardstick
           composed      the only composition available before: snapshot() +
                         GCDataset(...) + one sample (a record only; windows
                         of --composed-calls)

Windows, alternation, the two call styles and the statistics are
bench_replay.py's (bench_visual_sampler.window / stats), three alternating
rounds.  Conditions recorded with their numbers, each against the yardstick's
own round-to-round spread:

  add_step_no_slower_than_replay_add_step
      median(online) <= median(replay) + spread(replay) + 4 B x N / 1.0 TB/s
      (the ep_seq bytes at the rate DESIGN 4.11 measured for the insert:
      0.26 us at N = 65,536, 0.07 us at N = 16,384)
  sample_refill_no_slower_than_gcdataset_plain
      median(online refill) <= median(gc_plain refill) + spread(gc_plain refill)

  python scripts/bench_online_replay.py --out profiles/online_replay.json

--trace-worker runs 200 inserts and 200 samples at the pointmaze shape and
nothing else (for a profiler's kernel trace).
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import bench_visual_sampler as bv  # noqa: E402

ROWS = 1 << 22
BATCH = 1024
SHAPES = dict(pointmaze=dict(n=65536, ob=2, act=2), antmaze=dict(n=16384, ob=29, act=8))
STYLES = ('new', 'refill')
GCIQL = dict(bv.GCIQL, p_aug=None, frame_stack=None)
EP_SEQ_RATE = 1.0e6  # bytes per us: DESIGN 4.11, the insert's 6.8 MB in 6.6 us


def step_outputs(torch, shape, dev):
    """What a vectorized env's step hands out, with the caller's copy of the
    previous observation (bench_replay.step_outputs plus truncated)."""
    g = torch.Generator(device=dev).manual_seed(1)
    n, ob, act = shape['n'], shape['ob'], shape['act']
    r = lambda *s: torch.rand(*s, generator=g, device=dev, dtype=torch.float64)  # noqa: E731
    term = r(n) < 0.05
    trunc = r(n) < 0.10
    return dict(observations=r(n, ob), actions=r(n, act).float(), rewards=r(n).float(), terminated=term,
                truncated=trunc, next_observations=r(n, ob), final_observation=r(n, ob), done=term | trunc)


def new_ring(torch, shape, dev, seed=1, fill=True):
    import numpy as np

    from ogbench_amd.datasets import GCReplayBuffer

    n = shape['n']
    ex = dict(observations=np.zeros(shape['ob']), actions=np.zeros(shape['act'], np.float32),
              next_observations=np.zeros(shape['ob']), terminals=np.float32(0))
    buf = GCReplayBuffer.create(ex, n, ROWS // n, GCIQL, device=dev, seed=seed)
    if fill:  # past the horizon, episodes of about 50 steps ending at different steps
        g = torch.Generator(device=dev).manual_seed(2)
        obs = torch.rand(n, shape['ob'], generator=g, device=dev, dtype=torch.float64)
        act = torch.rand(n, shape['act'], generator=g, device=dev)
        for _ in range(buf.horizon + 7):
            done = torch.rand(n, generator=g, device=dev) < 0.02
            buf.add_step(obs, act, done, None, obs, obs)
    return buf


def new_replay(torch, shape, dev, same):
    import numpy as np

    from ogbench_amd.datasets import ReplayBuffer

    if same:
        ex = dict(observations=np.zeros(shape['ob']), actions=np.zeros(shape['act'], np.float32),
                  next_observations=np.zeros(shape['ob']), terminals=np.float32(0))
    else:
        ex = dict(observations=np.zeros(shape['ob']), actions=np.zeros(shape['act'], np.float32), rewards=0.0,
                  masks=1.0, next_observations=np.zeros(shape['ob']))
    rb = ReplayBuffer.create(ex, ROWS, device=dev, seed=1)
    rb.pointer, rb.size = 0, ROWS - 1
    return rb


def sample_callers(make):
    new, refill = make(), make()
    batch = refill.sample(BATCH)
    return {'new': lambda: new.sample(BATCH), 'refill': lambda: refill.sample(BATCH, out=batch)}


def measure_shape(torch, name, args):
    from ogbench_amd.datasets import Dataset, GCDataset, GCReplayBuffer

    dev = torch.device('cuda', 0)
    shape = SHAPES[name]
    n = shape['n']
    step = step_outputs(torch, shape, dev)
    ring = new_ring(torch, shape, dev, fill=False)
    sac = new_replay(torch, shape, dev, same=False)
    same = new_replay(torch, shape, dev, same=True)
    s = step
    same_rows = dict(observations=s['observations'], actions=s['actions'], next_observations=s['next_observations'],
                     terminals=s['done'])
    fns = {
        ('insert', 'online', 'new'): lambda: ring.add_step(s['observations'], s['actions'], s['terminated'],
                                                           s['truncated'], s['next_observations'],
                                                           s['final_observation']),
        ('insert', 'online_done', 'new'): lambda: ring.add_step(s['observations'], s['actions'], s['done'], None,
                                                                s['next_observations'], s['final_observation']),
        ('insert', 'replay', 'new'): lambda: sac.add_step(s['observations'], s['actions'], s['rewards'],
                                                          s['terminated'], s['next_observations'],
                                                          s['final_observation'], s['done']),
        ('insert', 'replay_same', 'new'): lambda: same.add_transitions(same_rows),
    }
    # the rows written are the composition's
    fns[('insert', 'online', 'new')]()
    want = torch.where(s['done'][:, None], s['final_observation'], s['next_observations'])
    assert torch.equal(ring['next_observations'][:n], want) and torch.equal(ring['terminals'][:n], s['done'].float())

    filled = new_ring(torch, shape, dev)  # the ring the samplers draw from; no insert touches it below
    snap = filled.snapshot()

    def ring_sampler():  # samplers of their own over the same columns and tables
        b = GCReplayBuffer(dict(filled), n, filled.horizon, GCIQL, device=dev, seed=2)
        b.ep_seq.copy_(filled.ep_seq)
        b.cur_seq.copy_(filled.cur_seq)
        b.ep_end.copy_(filled.ep_end)
        b._steps = b._ring.steps = filled.steps
        return b

    makers = dict(online=ring_sampler,
                  gc_ahead=lambda: GCDataset(snap, dict(GCIQL, lookahead=True), seed=2),
                  gc_plain=lambda: GCDataset(snap, dict(GCIQL, lookahead=False), seed=2))
    for v, make in makers.items():
        for style, f in sample_callers(make).items():
            fns[('sample', v, style)] = f
    # at one (seed, call) the ring and the sampler over its snapshot return the same batch
    a, b = ring_sampler().sample(BATCH), makers['gc_plain']().sample(BATCH)
    assert all(torch.equal(a[k], b[k]) for k in a if k != 'terminals')  # the snapshot's also mark the newest rows

    def composed():
        return GCDataset(Dataset(filled.snapshot()), GCIQL, seed=2).sample(BATCH)

    for f in fns.values():
        for _ in range(args.warmup):
            f()
    composed()
    times = {k: [] for k in fns}
    times[('sample', 'composed', 'new')] = []
    for _ in range(args.reps):  # alternate the variants
        for k, f in fns.items():
            times[k].append(bv.window(torch, f, args.calls))
        times[('sample', 'composed', 'new')].append(bv.window(torch, composed, args.composed_calls))
    res = {}
    for (op, v, style), us in times.items():
        res.setdefault(op, {}).setdefault(v, {})[style] = bv.stats(us)
    row = sum(v[0].numel() * v.element_size() for v in ring.values())
    res['insert_bytes_written'] = (row + 4) * n
    res['sample_bytes_written'] = (row + 2 * ring['observations'][0].numel() * 8 + 16) * BATCH
    ins, smp = res['insert'], res['sample']
    allowance = round(4 * n / EP_SEQ_RATE, 3)
    yard_i, yard_s = ins['replay']['new'], smp['gc_plain']['refill']
    cond = {
        'add_step_no_slower_than_replay_add_step': dict(
            online_us=ins['online']['new']['median_us'], replay_us=yard_i['median_us'],
            spread_replay_us=yard_i['spread_us'], ep_seq_allowance_us=allowance,
            holds=bool(ins['online']['new']['median_us'] <= yard_i['median_us'] + yard_i['spread_us'] + allowance)),
        'sample_refill_no_slower_than_gcdataset_plain': dict(
            online_us=smp['online']['refill']['median_us'], gc_plain_us=yard_s['median_us'],
            spread_gc_plain_us=yard_s['spread_us'], gc_ahead_us=smp['gc_ahead']['refill']['median_us'],
            holds=bool(smp['online']['refill']['median_us'] <= yard_s['median_us'] + yard_s['spread_us'])),
    }
    return dict(envs=n, horizon=ring.horizon, observation_dim=shape['ob'], action_dim=shape['act'], row_bytes=row,
                variants=res, conditions=cond)


def trace_worker():
    import torch

    dev = torch.device('cuda', 0)
    shape = SHAPES['pointmaze']
    s = step_outputs(torch, shape, dev)
    ring = new_ring(torch, shape, dev)
    batch = ring.sample(BATCH)
    for _ in range(200):
        ring.add_step(s['observations'], s['actions'], s['done'], None, s['next_observations'], s['final_observation'])
        ring.sample(BATCH, out=batch)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=2000, help='calls per timed window')
    ap.add_argument('--composed-calls', type=int, default=10, help='calls per window of the composed sample')
    ap.add_argument('--reps', type=int, default=3, help='alternating rounds (windows per variant)')
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--trace-worker', action='store_true', help='only run the two kernels at the pointmaze shape')
    args = ap.parse_args()
    if args.trace_worker:
        return trace_worker()
    import torch

    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    rec = dict(
        what='per-call time of GCReplayBuffer.add_step / sample(1024) against ReplayBuffer.add_step and '
             'GCDataset.sample(1024) over a static dataset of the same rows, host clock around windows of calls '
             'closed by a device synchronise',
        device=torch.cuda.get_device_name(0), ring_rows=ROWS, batch=BATCH, calls_per_window=args.calls,
        composed_calls_per_window=args.composed_calls, windows=args.reps,
        shapes={name: measure_shape(torch, name, args) for name in SHAPES})
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
