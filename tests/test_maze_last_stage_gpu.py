"""The point-maze step without its last RK stage's solve (point_contact.h, "the
last stage"): a step starts at rest and returns the position only, so the solve
of RK phase 3 of the last substep reaches nothing and both contact loops end
after that stage's position offsets.

A seeded batch of near-wall pointmaze-large envs (tests/last_stage_batch.py:
faces, inner corners, outer corners; float32 actions that push into the walls)
runs K = 8 consecutive steps at N = 1, 65 (one full wave and a wave of one env
with 63 copy lanes) and 4,096:

  * within 1e-9 of the oracle step, flags equal;
  * bit-identical at 8 / 16 / 32 / 64 envs per wave;
  * bit-identical between 8 env.step calls and one rollout of the 8 actions;
  * at least a tenth of the envs are in wall contact at the start of every
    step (the oracle's contact flag), so none of this passes on free space.

The structural check needs the mask-trace diagnostic build (one library per
process, so it runs scripts/probe_last_stage.py in a process of its own) and
skips where that build is absent.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ogbench_amd
from ogbench_amd import _lib
from last_stage_batch import K, MAZE, near_wall_batch, oracle_run

pytestmark = pytest.mark.gpu
TOL = 1e-9  # contact dynamics against the oracle, as tests/test_locomaze_gpu.py
SEED = 5
SIZES = (1, 65, 4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK_LIB = os.environ.get('OGBX_MASK_TRACE_LIB', os.path.join(ROOT, '_abx', 'libogbx_masks.so'))


def _env(gpu, n):
    return ogbench_amd.MazeEnv('point', MAZE, num_envs=n, device=gpu, auto_reset=True)


@functools.lru_cache(maxsize=None)
def _case(n):
    """The batch at size n as a state dict (host tensors), its actions, and the oracle's run of it."""
    dev = torch.device('cuda', 0)
    env = _env(dev, n)
    env.reset(seed=SEED, options=dict(task_id=torch.tensor((np.arange(n) % env.num_tasks + 1).astype(np.int32))))
    sd = {k: v.cpu() if torch.is_tensor(v) else v for k, v in env.state_dict().items()}
    env.close()
    q, acts, kind = near_wall_batch(n)
    sd['qpos'] = torch.tensor(q)
    ref, share, st = oracle_run(q, acts, sd['goal'].numpy(), sd['elapsed'].numpy(), sd['task'].numpy(),
                                sd['episode'].numpy(), SEED)
    return sd, acts, kind, ref, share, st


def _loaded(gpu, n, sd, epw=None):
    env = _env(gpu, n)
    if epw is not None:
        _lib.check(env._L.ogbx_maze_set_envs_per_wave(env._h, epw))
    env.reset(seed=SEED)
    env.load_state_dict(sd)  # copies the host tensors into the env's own state
    return env


def _steps(env, acts):
    """K env.step calls: per-step outputs [K, n, ...] and the final qpos."""
    rows = dict(obs=[], reward=[], terminated=[], truncated=[], success=[])
    for t in range(K):
        ob, rew, term, trunc, info = env.step(acts[t])
        for key, v in zip(rows, (ob, rew, term, trunc, info['success'])):
            rows[key].append(v.cpu().numpy().copy())
    out = {k: np.stack(v) for k, v in rows.items()}
    return out, env.state_dict()['qpos'].cpu().numpy()


@pytest.mark.parametrize('n', SIZES)
def test_matches_the_oracle_in_contact(gpu, n):
    sd, acts_np, kind, ref, share, st = _case(n)
    if n >= 3:
        assert set(np.unique(kind)) == {0, 1, 2}
    print('n = %d: share of envs in wall contact per step %s' % (n, np.round(share, 3)))
    assert (share >= 0.1).all(), share
    env = _loaded(gpu, n, sd)
    got, qpos = _steps(env, torch.tensor(acts_np, device=gpu))
    env.close()
    err = np.abs(got['obs'] - ref['obs']).max()
    print('n = %d: max |obs - oracle| = %.3e' % (n, err))
    assert err <= TOL
    assert np.abs(qpos - st['qpos']).max() <= TOL
    for key in ('terminated', 'truncated', 'success'):
        assert np.array_equal(got[key].astype(bool), ref[key].astype(bool)), key


@pytest.mark.parametrize('n', SIZES)
def test_bit_identical_across_envs_per_wave(gpu, n):
    sd, acts_np = _case(n)[:2]
    acts = torch.tensor(acts_np, device=gpu)
    res = {}
    for epw in (64, 32, 16, 8):
        env = _loaded(gpu, n, sd, epw)
        res[epw] = _steps(env, acts)
        env.close()
    for epw in (32, 16, 8):
        for key, v in res[epw][0].items():
            assert np.array_equal(v.view(np.uint8), res[64][0][key].view(np.uint8)), (epw, key)
        assert np.array_equal(res[epw][1].view(np.uint64), res[64][1].view(np.uint64)), epw


@pytest.mark.parametrize('n', SIZES)
def test_steps_equal_one_rollout(gpu, n):
    sd, acts_np = _case(n)[:2]
    acts = torch.tensor(acts_np, device=gpu)
    a, b = _loaded(gpu, n, sd), _loaded(gpu, n, sd)
    stepped, q_steps = _steps(a, acts)
    roll = {k: v.cpu().numpy() for k, v in b.rollout(acts).items()}
    q_roll = b.state_dict()['qpos'].cpu().numpy()
    a.close()
    b.close()
    assert np.array_equal(stepped['obs'].view(np.uint64), roll['obs'].view(np.uint64))
    assert np.array_equal(stepped['reward'].view(np.uint32), roll['reward'].view(np.uint32))
    for key in ('terminated', 'truncated', 'success'):
        assert np.array_equal(stepped[key].astype(bool), roll[key].astype(bool)), key
    assert np.array_equal(q_steps.view(np.uint64), q_roll.view(np.uint64))


@pytest.mark.skipif(not os.path.exists(MASK_LIB), reason='no mask-trace diagnostic build (scripts/build_maze_variant.sh '
                                                         'masks -DOGBX_MASK_TRACE)')
def test_no_active_set_iteration_at_the_last_stage(gpu):
    """With the mask-trace build: over the batch's 8 steps no env's last stage starts from one mask and settles on
    another or is flagged unsettled, while earlier stages of the same run do iterate (the trace is live)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'probe_last_stage.py')],
                       env=dict(os.environ, OGBX_LIB=MASK_LIB), capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert 'LAST_STAGE_CLEAN' in p.stdout
