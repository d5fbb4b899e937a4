#!/usr/bin/env python
"""Per-call time of the frame-stack push (include/ogbx_framestack.h) on the GPU.

Shares (k = 3 everywhere):
  powderworld  N = 4,096, observations uint8 [64, 64, 6]: stacks of 302 MB
  pointmaze    N = 65,536, observations float64 [2]
  antmaze      N = 16,384, observations float64 [29]
1 % of the envs are done per step (terminated and truncated masks, both
passed); the maze shares also compose a final stack, powderworld supplies no
final observation.  Variants:

  push           ogbx_framestack_push back to back, the two stacks alternating
  torch_compose  the yardstick: the best torch composition available before,
                 with preallocated outputs -- cat((prev[..., C:], obs), -1,
                 out=next), terminated | truncated, a where() over the k slots
                 for the done envs and a second cat for the final stack
  copy           the ceiling: copy_ of one stack-sized tensor, the same kF bytes
                 in and kF bytes out that push moves at its floor
  step / env_step  FrameStack.step and the bare env.step on two envs of the
                 share (pointmaze and powderworld; ant handles have no physics
                 here): their difference is what the wrapper adds to a step

Windows of back-to-back calls on the host clock, closed by a device
synchronise (bench_visual_sampler.window / stats), three alternating rounds,
medians, spread = max - min.  Conditions, each against the yardstick's or the
ceiling's own spread:

  push_no_slower_than_torch_compose   (every share)
      median(push) <= median(torch_compose) + spread(torch_compose)
  push_within_copy_spread_of_copy     (powderworld; reported with the fraction
      of the copy rate push reaches)
      median(push) <= median(copy) + spread(copy)

  python scripts/bench_framestack.py --out profiles/framestack.json

--trace-worker runs 200 pushes at the powderworld share and nothing else (for
a profiler's kernel trace).
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import bench_visual_sampler as bv  # noqa: E402

K = 3
DONE = 0.01
SHARES = dict(
    powderworld=dict(n=4096, frame=(64, 64, 6), dtype='uint8', final=False,
                     env=('powderworld-easy-v0', dict(world_size=64, auto_reset=True))),
    pointmaze=dict(n=65536, frame=(2,), dtype='float64', final=True,
                   env=('pointmaze-large-v0', dict(auto_reset=True))),
    antmaze=dict(n=16384, frame=(29,), dtype='float64', final=True, env=None),
)


def buffers(torch, share, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    n, frame, dtype = share['n'], share['frame'], getattr(torch, share['dtype'])

    def rnd(*shape):
        if dtype == torch.uint8:
            return torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8)
        return torch.rand(*shape, generator=g, device=dev, dtype=dtype)

    stacked = (n,) + frame[:-1] + (frame[-1] * K,)
    u = torch.rand(n, generator=g, device=dev)
    return dict(obs=rnd(n, *frame), final_obs=rnd(n, *frame), stacks=[rnd(*stacked), rnd(*stacked)],
                final=rnd(*stacked), term=(u < DONE / 2).to(torch.uint8),
                trunc=((u >= DONE / 2) & (u < DONE)).to(torch.uint8), copy_dst=torch.empty(stacked, dtype=dtype,
                                                                                          device=dev))


def push_caller(torch, share, b):
    """ogbx_framestack_push on raw pointers, as FrameStack.step calls it."""
    from ogbench_amd import _framestack, _lib

    L = _framestack.bind()
    shape = _framestack.shape_of(b['obs'], K)
    ptrs = [s.data_ptr() for s in b['stacks']]
    obs, term, trunc = b['obs'].data_ptr(), b['term'].data_ptr(), b['trunc'].data_ptr()
    fobs, final = (b['final_obs'].data_ptr(), b['final'].data_ptr()) if share['final'] else (None, None)
    raw_stream, state = torch._C._cuda_getCurrentRawStream, [0]

    def call():
        cur = state[0]
        st = L.ogbx_framestack_push(shape, obs, ptrs[cur], term, trunc, fobs, ptrs[1 - cur], final, raw_stream(0))
        if st:
            _lib.check(st, 'framestack_push')
        state[0] = 1 - cur

    return call


def torch_caller(torch, share, b):
    c = share['frame'][-1]
    stacks, obs, final_obs, final = b['stacks'], b['obs'], b['final_obs'], b['final']
    term, trunc = b['term'].view(torch.bool), b['trunc'].view(torch.bool)
    lead = (-1,) + (1,) * (len(share['frame']) + 1)  # done over [N, ..., k, C]
    slots = [s.view(s.shape[:-1] + (K, c)) for s in stacks]
    obs_slot = obs.unsqueeze(-2)
    state = [0]

    def call():
        cur = state[0]
        prev, nxt = stacks[cur], stacks[1 - cur]
        torch.cat((prev[..., c:], obs), -1, out=nxt)
        done = (term | trunc).view(lead)
        torch.where(done, obs_slot, slots[1 - cur], out=slots[1 - cur])
        if share['final']:
            torch.cat((prev[..., c:], final_obs), -1, out=final)
        state[0] = 1 - cur

    return call


def check_equal(torch, share, b):
    """push and the torch composition write the same stacks."""
    from ogbench_amd import _framestack

    prev = b['stacks'][0].clone()
    torch_caller(torch, share, dict(b, stacks=[prev.clone(), b['stacks'][1]]))()
    want, want_final = b['stacks'][1].clone(), b['final'].clone()
    nxt, final = torch.empty_like(prev), torch.zeros_like(prev)
    _framestack.push(_framestack.shape_of(b['obs'], K), b['obs'], prev, b['term'], b['trunc'],
                     b['final_obs'] if share['final'] else None, nxt, final if share['final'] else None)
    done = (b['term'] | b['trunc']).bool()
    assert torch.equal(nxt, want), 'push and the torch composition disagree'
    assert not share['final'] or torch.equal(final[done], want_final[done])
    return int(done.sum())


def env_callers(torch, share, dev):
    import ogbench_amd
    from ogbench_amd.wrappers import FrameStack

    env_id, kw = share['env']
    n = share['n']
    bare = ogbench_amd.make(env_id, num_envs=n, device=dev, **kw)
    wrapped = FrameStack(ogbench_amd.make(env_id, num_envs=n, device=dev, **kw), K)
    bare.reset(seed=1)
    wrapped.reset(seed=1)
    if 'powder' in env_id:
        action = torch.zeros(n, dtype=torch.int32, device=dev)
    else:
        action = (torch.rand(n, 2, device=dev) * 2 - 1).float()
    return {'env_step': lambda: bare.step(action), 'step': lambda: wrapped.step(action)}


def measure_share(torch, name, args):
    dev = torch.device('cuda', 0)
    share = SHARES[name]
    b = buffers(torch, share, dev)
    n_done = check_equal(torch, share, b)
    src, dst = b['stacks'][0], b['copy_dst']
    fns = {'push': push_caller(torch, share, b), 'torch_compose': torch_caller(torch, share, b),
           'copy': lambda: dst.copy_(src)}
    if share['env'] is not None:
        fns.update(env_callers(torch, share, dev))
    calls = args.calls if name != 'powderworld' else args.powder_calls
    for f in fns.values():
        for _ in range(args.warmup):
            f()
    times = {k: [] for k in fns}
    for _ in range(args.reps):  # alternate the variants
        for k, f in fns.items():
            times[k].append(bv.window(torch, f, calls))
    res = {k: bv.stats(us) for k, us in times.items()}
    stack_bytes = src.numel() * src.element_size()
    obs_bytes = b['obs'].numel() * b['obs'].element_size()
    push, yard, copy = res['push'], res['torch_compose'], res['copy']
    rate = lambda us: round(2 * stack_bytes / us / 1e3, 1)  # noqa: E731  (GB/s: bytes read + bytes written)
    out = dict(envs=share['n'], frame=list(share['frame']), dtype=share['dtype'], num_stack=K, done_envs=n_done,
               final_stack=share['final'], calls_per_window=calls, stack_bytes=stack_bytes,
               frame_bytes=obs_bytes, variants=res,
               push_GBps=rate(push['median_us']), copy_GBps=rate(copy['median_us']))
    if 'step' in res:
        out['step_minus_env_step_us'] = round(res['step']['median_us'] - res['env_step']['median_us'], 3)
    cond = {'push_no_slower_than_torch_compose': dict(
        push_us=push['median_us'], torch_compose_us=yard['median_us'], spread_torch_compose_us=yard['spread_us'],
        verdict='PASS' if push['median_us'] <= yard['median_us'] + yard['spread_us'] else 'FAIL')}
    if name == 'powderworld':
        holds = push['median_us'] <= copy['median_us'] + copy['spread_us']
        cond['push_within_copy_spread_of_copy'] = dict(
            push_us=push['median_us'], copy_us=copy['median_us'], spread_copy_us=copy['spread_us'],
            push_fraction_of_copy_rate=round(copy['median_us'] / push['median_us'], 3),
            below_copy_by_us=round(max(0.0, push['median_us'] - copy['median_us'] - copy['spread_us']), 3),
            verdict='PASS' if holds else 'FAIL')
    out['conditions'] = cond
    return out


def trace_worker():
    import torch

    dev = torch.device('cuda', 0)
    share = SHARES['powderworld']
    call = push_caller(torch, share, buffers(torch, share, dev))
    for _ in range(200):
        call()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=2000, help='calls per timed window (maze shares)')
    ap.add_argument('--powder-calls', type=int, default=200, help='calls per timed window (powderworld share)')
    ap.add_argument('--reps', type=int, default=3, help='alternating rounds (windows per variant)')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--shares', default=','.join(SHARES))
    ap.add_argument('--out', default=None, help='write the JSON record here (default: print only)')
    ap.add_argument('--trace-worker', action='store_true', help='only run push at the powderworld share')
    args = ap.parse_args()
    if args.trace_worker:
        return trace_worker()
    import torch

    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    rec = dict(
        what='per-call time of ogbx_framestack_push against the torch composition it replaces and a copy_ of one '
             'stack, host clock around windows of back-to-back calls closed by a device synchronise',
        device=torch.cuda.get_device_name(0), windows=args.reps,
        shares={name: measure_share(torch, name, args) for name in args.shares.split(',')})
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
