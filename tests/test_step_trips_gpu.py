"""The lean contact loop's active-set trips (point_contact.h: piece weights from
the edge activities, the first trip in line ahead of the rolled loop) on states
that iterate: every env starts in a corner or against a wall end -- two or
three walls among the face, face and diagonal boxes of its side, offsets
1.3-1.9 from the cell centre on both axes -- and is pushed with f64 actions of
full magnitude for 12 steps, so stick/slip flips happen in most stages.

  * the plain instantiation (env.step's launch, 64 envs per wave) against the
    generic one at 8 envs per wave: outputs and state bit for bit -- a lane's
    result does not depend on how many trips the other lanes of its wave need.
    This is the comparison that covers a settled lane's rerun (the lanes that
    share a wave differ between the two, so a lane settled while its
    neighbours iterate in one of them is not in the other);
  * both within 1e-9 of the oracle;
  * 64 copies of one such env in one wave: every lane's result equals lane 0's
    (all lanes take the same trips here, so this checks only that no lane's
    result depends on its position in the wave).

The results are bit-equal to the previous loop's, so the file is a regression
test of the trips' path, not of a new result.
"""
import numpy as np
import pytest
import torch

import ogbench_amd
from ogbench_amd import _lib
from oracle import locomaze as orc

pytestmark = pytest.mark.gpu
TOL = 1e-9  # contact dynamics against the oracle, as tests/test_locomaze_gpu.py
K, N, SEED = 12, 257, 5
OUT_KEYS = ('obs', 'reward', 'terminated', 'truncated', 'success', 'final_obs')
STATE_KEYS = ('qpos', 'goal', 'elapsed', 'task', 'episode')


def _env(gpu, n, maze, auto_reset=True):
    return ogbench_amd.MazeEnv('point', maze, num_envs=n, device=gpu, auto_reset=auto_reset)


def _corner_starts(maze, n, rng):
    """n start positions, each 1.3-1.9 from its cell's centre on both axes towards
    a side (sx, sy) whose three boxes hold two or three walls; the wall count of each."""
    mp, _ = orc.tables(maze)
    spots = []
    for i, j in np.argwhere(mp == 0):
        for sx in (-1, 1):
            for sy in (-1, 1):
                walls = int(mp[i, j + sx]) + int(mp[i + sy, j]) + int(mp[i + sy, j + sx])
                if walls >= 2:
                    spots.append((i, j, sx, sy, walls))
    spots = np.array(spots)
    assert (spots[:, 4] == 2).any() and (spots[:, 4] == 3).any()
    pick = spots[rng.randint(len(spots), size=n)]
    # both kinds are present whatever the draw
    pick[0] = spots[spots[:, 4] == 3][0]
    pick[1] = spots[spots[:, 4] == 2][0]
    off = rng.uniform(1.3, 1.9, (n, 2))
    q = np.stack([pick[:, 1] * 4.0 - 4.0 + pick[:, 2] * off[:, 0], pick[:, 0] * 4.0 - 4.0 + pick[:, 3] * off[:, 1]], 1)
    return q, pick[:, 4]


def _start(gpu, maze, n, rng):
    env = _env(gpu, n, maze)
    tid = torch.tensor((np.arange(n) % env.num_tasks + 1).astype(np.int32))
    env.reset(seed=SEED, options=dict(task_id=tid))
    sd = env.state_dict()
    env.close()
    q, walls = _corner_starts(maze, n, rng)
    sd['qpos'] = torch.tensor(q, device=gpu)
    acts = rng.choice([-1.0, 1.0], size=(K, n, 2)).astype(np.float64)  # full magnitude on both axes
    return sd, acts, walls


def _loaded(gpu, n, maze, sd, auto_reset=True):
    env = _env(gpu, n, maze, auto_reset)
    env.reset(seed=SEED)
    env.load_state_dict(sd)
    return env


def _state(env):
    sd = env.state_dict()
    return {k: sd[k].cpu().numpy() for k in STATE_KEYS}


def _buffers(n, dev):
    return dict(obs=torch.zeros((n, 2), dtype=torch.float64, device=dev),
                reward=torch.zeros((n,), dtype=torch.float32, device=dev),
                terminated=torch.zeros((n,), dtype=torch.uint8, device=dev),
                truncated=torch.zeros((n,), dtype=torch.uint8, device=dev),
                success=torch.zeros((n,), dtype=torch.uint8, device=dev),
                final_obs=torch.zeros((n, 2), dtype=torch.float64, device=dev))


def _steps(env, acts, generic):
    """K single steps: env.step's bound launch, or the generic instantiation at 8 envs per wave."""
    out = _buffers(env.num_envs, env.device)
    ptrs = [_lib.ptr(out[k]) for k in OUT_KEYS]
    if generic:
        _lib.check(env._L.ogbx_maze_set_envs_per_wave(env._h, 8))
    else:
        _lib.check(env._L.ogbx_maze_bind_step(env._h, *ptrs, 1))
    outs, states = [], []
    for t in range(K):
        out['final_obs'].zero_()
        a = acts[t].contiguous()
        if generic:
            _lib.check(env._L.ogbx_maze_step(env._h, _lib.ptr(a), 1, 1, *ptrs, 1, env._stream()))
        else:
            _lib.check(env._L.ogbx_maze_step_bound(env._h, _lib.ptr(a), 1, env._stream()))
        outs.append({k: v.cpu().numpy().copy() for k, v in out.items()})
        states.append(_state(env))
    return outs, states


def _oracle(maze, sd, acts):
    st = dict(qpos=sd['qpos'].cpu().numpy().copy(), goal=sd['goal'].cpu().numpy().copy(),
              elapsed=sd['elapsed'].cpu().numpy().copy(), task=sd['task'].cpu().numpy().copy(),
              episode=sd['episode'].cpu().numpy().view(np.uint32).copy(), opts=orc._opts())
    return orc.step(maze, st, acts, auto_reset=1, key=orc.philox_key(SEED, orc.TAG_MAZE_RESET)), st


@pytest.mark.parametrize('maze', ['medium', 'large'])
def test_trips_plain_equals_generic_and_oracle(gpu, maze):
    rng = np.random.RandomState(300 + len(maze))
    sd, acts_np, walls = _start(gpu, maze, N, rng)
    assert set(np.unique(walls)) == {2, 3}
    # most envs are in contact at the first step (the action moves the env before the contact test)
    _, contact = orc.physics(maze, sd['qpos'].cpu().numpy(), acts_np[0])
    assert contact.sum() * 2 > N
    acts = torch.tensor(acts_np, device=gpu)
    e_plain, e_gen = _loaded(gpu, N, maze, sd), _loaded(gpu, N, maze, sd)
    plain, plain_states = _steps(e_plain, acts, generic=False)
    gen, gen_states = _steps(e_gen, acts, generic=True)
    e_plain.close()
    e_gen.close()
    for t in range(K):
        for key in OUT_KEYS:
            assert np.array_equal(plain[t][key].view(np.uint8), gen[t][key].view(np.uint8)), (key, t)
        for key in STATE_KEYS:
            assert np.array_equal(plain_states[t][key].view(np.uint8), gen_states[t][key].view(np.uint8)), (key, t)
    ref, st = _oracle(maze, sd, acts_np)
    for outs, states in ((plain, plain_states), (gen, gen_states)):
        err = np.abs(np.stack([p['obs'] for p in outs]) - ref['obs']).max()
        print('%s: max |obs - oracle| = %.3e' % (maze, err))
        assert err <= TOL
        assert np.abs(states[-1]['qpos'] - st['qpos']).max() <= TOL
        for key in ('terminated', 'truncated', 'success'):
            assert np.array_equal(np.stack([p[key] for p in outs]).astype(bool), ref[key].astype(bool)), key


def test_copies_of_one_env_agree_in_a_wave(gpu):
    """One wave of 64 copies of a three-wall corner env: every lane computes what lane 0 computes, bit for bit."""
    maze, n = 'large', 64
    rng = np.random.RandomState(77)
    sd, acts_np, walls = _start(gpu, maze, n, rng)
    assert walls[0] == 3
    for k in STATE_KEYS:
        sd[k] = sd[k][:1].expand(n, *sd[k].shape[1:]).contiguous()
    acts = torch.tensor(np.repeat(acts_np[:, :1], n, axis=1), device=gpu)
    _, contact = orc.physics(maze, sd['qpos'].cpu().numpy(), acts_np[0, :1].repeat(n, axis=0))
    assert contact.all()
    # no auto-reset: a reset would draw per env
    env = _loaded(gpu, n, maze, sd, auto_reset=False)
    for t in range(K):
        ob = env.step(acts[t])[0].cpu().numpy()
        q = env.state_dict()['qpos'].cpu().numpy()
        assert (ob.view(np.uint64) == ob.view(np.uint64)[0]).all(), t
        assert (q.view(np.uint64) == q.view(np.uint64)[0]).all(), t
    env.close()
