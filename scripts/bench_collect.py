"""A/B of point-maze data collection on one MI355X: the stepwise launches
against the fused collector (profiles/collect_fused_ab.txt).

Times datagen.collect_locomaze('pointmaze-large-v0', 'navigate',
max_episode_steps=1001) with fused=False (one expert_action, step, randint and
set_goal launch per step plus four strided copies, and the final permute) and
with fused=True (ceil(T / chunk) launches of maze_collect_kernel writing the
rows in place), at every batch size of --n.  Both run in one process,
alternating; one untimed warm-up each, then --repeats timed runs each; host
clock around the whole call (env creation, resets and the dataset's allocation
included), synchronised before and after.

Usage: python scripts/bench_collect.py [--n 1024,65536] [--t 1001] [--repeats 3]
                                       [--out profiles/collect_fused_ab.txt]
"""

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', default='1024,65536')
    ap.add_argument('--t', type=int, default=1001)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--env', default='pointmaze-large-v0')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'collect_fused_ab.txt'))
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error('--repeats must be at least 3')

    import torch

    from ogbench_amd.datagen import collect_locomaze

    dev = torch.device('cuda', 0)
    sync = torch.cuda.synchronize

    def run(n, fused, seed):
        sync()
        t0 = time.perf_counter()
        d = collect_locomaze(a.env, 'navigate', num_envs=n, max_episode_steps=a.t, seed=seed, device=dev, fused=fused,
                             chunk=a.chunk)
        sync()
        dt = time.perf_counter() - t0
        del d
        return dt

    lines = [f'collect_locomaze({a.env!r}, "navigate", max_episode_steps={a.t}), chunk {a.chunk}: stepwise '
             f'(fused=False) against fused (fused=True)',
             f'device: {torch.cuda.get_device_name(0)}; one process, alternating; 1 warm-up + {a.repeats} timed runs '
             f'each; seconds per call (host clock, synchronised before and after)', '']
    for n in (int(v) for v in a.n.split(',')):
        times = {False: [], True: []}
        for fused in (False, True):
            run(n, fused, 0)  # warm-up
        for r in range(a.repeats):
            for fused in (False, True):
                times[fused].append(run(n, fused, r + 1))
        s, f = times[False], times[True]
        ms, mf = statistics.median(s), statistics.median(f)
        steps = n * a.t
        lines += [f'num_envs = {n}  ({steps} env-steps per call)',
                  f'  stepwise  runs {" ".join(f"{x:.4f}" for x in s)}  median {ms:.4f}  spread (max - min) '
                  f'{max(s) - min(s):.4f}  {steps / ms / 1e6:.2f} M env-steps/s',
                  f'  fused     runs {" ".join(f"{x:.4f}" for x in f)}  median {mf:.4f}  spread (max - min) '
                  f'{max(f) - min(f):.4f}  {steps / mf / 1e6:.2f} M env-steps/s',
                  f'  stepwise / fused (medians) = {ms / mf:.2f}; difference of medians {ms - mf:.4f} s against a '
                  f'stepwise spread of {max(s) - min(s):.4f} s: fused is '
                  f'{"faster by more than" if ms - mf > max(s) - min(s) else "NOT faster by more than"} the spread', '']
        print('\n'.join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines))


if __name__ == '__main__':
    main()
