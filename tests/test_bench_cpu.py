"""CPU: bench.py's host-side helpers -- the traffic record is used only for a
run of the same workload, per-launch units and world size (else null), and the
sharding of the metric's fixed total N."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ogbench_amd.sharding import shard  # noqa: E402


def test_traffic_record_selected_by_configuration():
    with open(os.path.join(ROOT, 'profiles', 'traffic.json')) as f:
        rec = json.load(f)['maze_step_kernel@pointmaze']
    assert bench._traffic('maze_step_kernel', 'pointmaze', rec['units'], rec.get('world', 1)) == \
        rec['hbm_bytes_per_launch']
    assert bench._traffic('maze_step_kernel', 'pointmaze', rec['units'] // 2, 1) is None  # other N
    assert bench._traffic('maze_step_kernel', 'pointmaze', rec['units'], 2) is None  # other world size
    assert bench._traffic('maze_step_kernel', 'powder', rec['units'], 1) is None  # other workload
    # the committed record is within 1.15x of the 87 B/env-step algorithmic
    # bytes plus the kernel's instruction fetch: the fully unrolled contact
    # loop is 348 KB of code (86 KB at unroll 4, where the record was 1.06x),
    # fetched again every launch (the FETCH_SIZE pass grows by
    # 355 KiB per launch between the two builds)
    code_fetch = 2 * 355 * 1024
    assert rec['hbm_bytes_per_launch'] <= 1.15 * 87 * rec['units'] + code_fetch


def test_rank_layout_checks():
    # no launcher: one GPU runs in-process, N > 1 self-launches
    assert bench._check_world(1, 'gloo', env={}) == 'rank'
    assert bench._check_world(2, 'gloo', env={}) == 'self-launch'
    assert bench._check_world(2, 'gloo', env={'WORLD_SIZE': '2'}) == 'rank'
    # a launcher whose world size differs from --gpus is refused, not noted
    with pytest.raises(SystemExit) as e:
        bench._check_world(8, 'gloo', env={'WORLD_SIZE': '2'})
    assert e.value.code == 2
    # more RCCL ranks than visible GPUs (none here) is refused
    with pytest.raises(SystemExit) as e:
        bench._check_world(torch.cuda.device_count() + 1, 'nccl', env={})
    assert e.value.code == 2


def test_mismatched_world_exits_before_touching_the_gpu():
    env = dict(os.environ, WORLD_SIZE='3', RANK='0', LOCAL_RANK='0')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dist-backend', 'gloo'],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, (out.returncode, out.stderr[-2000:])
    assert 'WORLD_SIZE=3' in out.stderr and not any(ln.startswith('{') for ln in out.stdout.splitlines())


def test_self_launch_returns_the_worst_rank_status(tmp_path, monkeypatch):
    # the launcher itself, on a stand-in script: every rank sees its own
    # RANK / WORLD_SIZE and a shared 127.0.0.1 rendezvous, and the parent
    # returns the worst status
    probe = tmp_path / 'rank.py'
    probe.write_text('import os, sys\n'
                     'print(os.environ["RANK"], os.environ["WORLD_SIZE"], os.environ["MASTER_ADDR"], flush=True)\n'
                     'sys.exit(3 if os.environ["RANK"] == "1" else 0)\n')
    monkeypatch.setattr(bench, '__file__', str(probe))
    rc, rcs = bench._self_launch(3, [])
    assert rcs == [0, 3, 0] and rc == 3


def test_strong_scaling_shards_cover_the_total():
    for world in (1, 2, 4, 8):
        spans = [shard(65536, world, r) for r in range(world)]
        assert spans[0][0] == 0 and sum(n for _, n in spans) == 65536
        for (b0, n0), (b1, _) in zip(spans, spans[1:]):
            assert b0 + n0 == b1
        assert all(n % 64 == 0 for _, n in spans)  # whole waves per rank


def test_dump_outputs_names_dtypes_and_fixed_sample(tmp_path):
    # a step tuple: info's tensors are flattened, 64-bit values stay 64-bit,
    # everything else is stored as float32
    g = torch.Generator().manual_seed(0)
    obs = torch.rand(1000, 4, dtype=torch.float64, generator=g)
    ret = (obs, torch.rand(1000, generator=g), torch.arange(1000) % 3 == 0, torch.zeros(1000, dtype=torch.bool),
           {'success': torch.arange(1000) % 2 == 0, 'note': 'not a tensor'})
    shapes = bench._dump_outputs(str(tmp_path / 'all'), ret)
    assert shapes == {'obs': [1000, 4], 'reward': [1000], 'terminated': [1000], 'truncated': [1000],
                      'info_success': [1000]}
    got = {k: np.load(tmp_path / 'all' / f'{k}.npy') for k in shapes}
    assert got['obs'].dtype == np.float64 and np.array_equal(got['obs'], obs.numpy())
    assert got['reward'].dtype == np.float32 and np.array_equal(got['reward'], ret[1].numpy())
    assert got['terminated'].dtype == np.float32 and np.array_equal(got['terminated'], ret[2].numpy())
    # over the size limit: the same seeded rows of every array, the same on every call, within the limit
    limit = 8000
    s1 = bench._dump_outputs(str(tmp_path / 's1'), ret, limit=limit)
    s2 = bench._dump_outputs(str(tmp_path / 's2'), ret, limit=limit)
    assert s1 == s2 and 1 < s1['obs'][0] < 1000 and s1['obs'][0] == s1['reward'][0]
    sub = {k: np.load(tmp_path / 's1' / f'{k}.npy') for k in s1}
    assert sum(v.nbytes for v in sub.values()) <= limit
    for k in sub:
        assert np.array_equal(sub[k], np.load(tmp_path / 's2' / f'{k}.npy'))
    rows = np.flatnonzero((obs.numpy()[:, None, :] == sub['obs'][None]).all(-1).any(1))
    assert len(rows) == s1['obs'][0] and np.array_equal(sub['reward'], ret[1].numpy()[rows])
    # a sampler's batch dict, several ranks: one file per name and rank
    bench._dump_outputs(str(tmp_path / 'r'), {'actor/goals': torch.ones(3, 2), 'idxs': torch.arange(3)}, rank=1, world=2)
    assert sorted(os.listdir(tmp_path / 'r')) == ['actor_goals.rank1.npy', 'idxs.rank1.npy']
    assert np.load(tmp_path / 'r' / 'idxs.rank1.npy').dtype == np.float64


def test_plain_run_switches_everything_else_off(monkeypatch):
    # without --full the parsed options ask for no extras and no CPU baseline
    seen = {}

    def fake(args, world, rank, dev):
        seen.update(vars(args))
        raise SystemExit(0)

    monkeypatch.setattr(bench, 'bench_pointmaze', fake)
    monkeypatch.setattr(bench, '_dist_init', lambda backend: (1, 0, 0))
    for argv, full in ((['--steps', '7'], False), (['--steps', '7', '--full'], True)):
        with pytest.raises(SystemExit):
            bench.main(argv + ['--dist-backend', 'gloo'])  # (the nccl layout check wants a visible GPU)
        assert seen['steps'] == 7 and seen['full'] is full
        assert seen['no_extras'] is (not full) and seen['no_cpu_baseline'] is (not full)
