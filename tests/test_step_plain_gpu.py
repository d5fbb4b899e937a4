"""The plain single-step instantiation of maze_step_kernel (what env.step
launches: k_steps = 1, 64 envs per wave, no teleports) against the generic
one, bit for bit, and the instantiations the launcher picks for a teleport
maze and a success_timing='pre' env against the oracle.

Shapes: N = 1, 63, 64 and 64*3 + 5 (a partial wave, a full wave, a partial
block); f32 and f64 actions; near-wall starts so that contact and bail paths
run; 30 steps with TimeLimit auto-resets (elapsed starts at max_steps - 3),
envs that start within goal_tol of their goal (success, terminate, auto-reset
with final_obs) and one env whose first action, of magnitude 50 (outside the
action space), lands it on its goal from 10 units away -- the env the
prologue's near-goal prefetch does not cover.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import ogbench_amd
from ogbench_amd import _lib
from oracle import locomaze as orc

pytestmark = pytest.mark.gpu
TOL = 1e-9  # contact dynamics against the oracle, as tests/test_locomaze_gpu.py
K, MAX_STEPS, SEED = 30, 11, 5
SENTINEL = -7.0


def _env(gpu, n, maze, **kw):
    kw.setdefault('max_episode_steps', MAX_STEPS)
    return ogbench_amd.MazeEnv('point', maze, num_envs=n, device=gpu, auto_reset=True, **kw)


def _start(gpu, maze, n, f64, rng, **kw):
    """Start state (near walls / near goals / one far env) and K actions."""
    env = _env(gpu, n, maze, **kw)
    tid = torch.tensor((np.arange(n) % 5 + 1).astype(np.int32))
    env.reset(seed=SEED, options=dict(task_id=tid))
    sd = env.state_dict()
    goal = sd['goal'].cpu().numpy()
    mp, _ = orc.tables(maze)
    cells = np.argwhere(mp == 0)
    c = cells[rng.randint(len(cells), size=n)]
    q = np.stack([c[:, 1] * 4.0 - 4 + rng.uniform(-1.9, 1.9, n), c[:, 0] * 4.0 - 4 + rng.uniform(-1.9, 1.9, n)], 1)
    near = np.arange(n) % 7 == 3
    q[near] = goal[near] + rng.uniform(-0.3, 0.3, (int(near.sum()), 2))
    acts = rng.uniform(-1, 1, (K, n, 2))
    far = n // 2
    q[far] = goal[far] + [-10.0, 0.0]
    acts[0, far] = [50.0, 0.0]
    acts = acts.astype(np.float64 if f64 else np.float32)
    sd['qpos'] = torch.tensor(q, device=gpu)
    sd['elapsed'] = torch.full((n,), MAX_STEPS - 3, dtype=torch.int32, device=gpu)
    env.close()
    return sd, acts, far


def _oracle(maze, sd, acts, **opts):
    st = dict(qpos=sd['qpos'].cpu().numpy().copy(), goal=sd['goal'].cpu().numpy().copy(),
              elapsed=sd['elapsed'].cpu().numpy().copy(), task=sd['task'].cpu().numpy().copy(),
              episode=sd['episode'].cpu().numpy().view(np.uint32).copy(), opts=orc._opts(max_steps=MAX_STEPS, **opts))
    ref = orc.step(maze, st, acts, auto_reset=1, key=orc.philox_key(SEED, orc.TAG_MAZE_RESET))
    return ref, st


def _state(env):
    sd = env.state_dict()
    return {k: sd[k].cpu().numpy() for k in ('qpos', 'goal', 'elapsed', 'task', 'episode')}


def _bound_steps(env, acts):
    """K calls of env.step (the bound single step); outputs and state after each."""
    outs, states = [], []
    for t in range(K):
        env._final_obs.fill_(SENTINEL)
        ob, rew, term, trunc, info = env.step(acts[t])
        outs.append(dict(obs=ob.cpu().numpy().copy(), reward=rew.cpu().numpy().copy(),
                         terminated=term.cpu().numpy().copy(), truncated=trunc.cpu().numpy().copy(),
                         success=info['success'].cpu().numpy().copy(),
                         final_obs=info['final_observation'].cpu().numpy().copy()))
        states.append(_state(env))
    return outs, states


def _abi_steps(env, acts):
    """The same steps through ogbx_maze_step with k_steps = 1."""
    n, dev = env.num_envs, env.device
    buf = dict(obs=torch.empty(n, 2, dtype=torch.float64, device=dev),
               reward=torch.empty(n, dtype=torch.float32, device=dev),
               terminated=torch.empty(n, dtype=torch.uint8, device=dev),
               truncated=torch.empty(n, dtype=torch.uint8, device=dev),
               success=torch.empty(n, dtype=torch.uint8, device=dev),
               final_obs=torch.empty(n, 2, dtype=torch.float64, device=dev))
    outs, states = [], []
    for t in range(K):
        buf['final_obs'].fill_(SENTINEL)
        a = acts[t].contiguous()
        _lib.check(env._L.ogbx_maze_step(env._h, _lib.ptr(a), int(a.dtype == torch.float64), 1, _lib.ptr(buf['obs']),
                                         _lib.ptr(buf['reward']), _lib.ptr(buf['terminated']),
                                         _lib.ptr(buf['truncated']), _lib.ptr(buf['success']),
                                         _lib.ptr(buf['final_obs']), 1, env._stream()))
        outs.append({k: v.cpu().numpy().copy() for k, v in buf.items()})
        states.append(_state(env))
    return outs, states


@pytest.mark.parametrize('n', [1, 63, 64, 64 * 3 + 5])
@pytest.mark.parametrize('f64', [False, True])
@pytest.mark.parametrize('maze', ['medium', 'large'])
def test_plain_step_equals_generic_paths(gpu, maze, f64, n):
    rng = np.random.RandomState(1000 * n + 2 * sum(map(ord, maze)) + int(f64))
    sd, acts_np, far = _start(gpu, maze, n, f64, rng)
    acts = torch.tensor(acts_np, device=gpu)
    envs = [_env(gpu, n, maze) for _ in range(3)]
    for e in envs:
        e.reset(seed=SEED)
        e.load_state_dict(sd)
    plain, plain_states = _bound_steps(envs[0], acts)
    # generic: one step per launch at 32 envs per wave
    _lib.check(envs[1]._L.ogbx_maze_set_envs_per_wave(envs[1]._h, 32))
    gen, gen_states = _abi_steps(envs[1], acts)
    for t in range(K):
        for key in plain[t]:
            got, want = plain[t][key], gen[t][key].astype(plain[t][key].dtype)
            assert np.array_equal(got, want), (key, t)
        for key in plain_states[t]:
            assert np.array_equal(plain_states[t][key], gen_states[t][key]), (key, t)
    # generic: the K steps in one launch
    roll = {k: v.cpu().numpy() for k, v in envs[2].rollout(acts).items()}
    for key in ('obs', 'reward', 'terminated', 'truncated', 'success'):
        stacked = np.stack([plain[t][key] for t in range(K)])
        assert np.array_equal(stacked, roll[key].astype(stacked.dtype)), key
    last = _state(envs[2])
    for key in last:
        assert np.array_equal(plain_states[-1][key], last[key]), key
    # and the steps are the right ones: the oracle, with the events the shapes are chosen for
    ref, st = _oracle(maze, sd, acts_np)
    obs = np.stack([p['obs'] for p in plain])
    assert np.abs(obs - ref['obs']).max() <= TOL
    for key in ('terminated', 'truncated', 'success'):
        assert np.array_equal(np.stack([p[key] for p in plain]).astype(bool), ref[key].astype(bool)), key
    assert np.array_equal(np.stack([p['reward'] for p in plain]), ref['reward'])
    assert np.array_equal(plain_states[-1]['episode'].view(np.uint32), st['episode'])
    running = ~ref['terminated'][:3].astype(bool).any(0)  # no goal reset before the TimeLimit at step 2
    assert ref['truncated'][2][running].all() and ref['truncated'].sum() >= n
    assert ref['success'][0, far] == 1 and ref['terminated'][0, far] == 1
    assert np.abs(plain[0]['final_obs'][far] - sd['goal'].cpu().numpy()[far]).max() < 1e-5
    assert ref['success'][0].sum() >= max(n // 7, 1)  # the far env and the near-goal envs
    ended = (ref['terminated'] | ref['truncated']).astype(bool)
    fin = np.stack([p['final_obs'] for p in plain])
    assert (fin[~ended] == SENTINEL).all() and (fin[ended] != SENTINEL).all()
    for e in envs:
        e.close()


@pytest.mark.parametrize('variant', ['teleport', 'success_pre'])
def test_launcher_choice_matches_oracle(gpu, variant):
    """A teleport maze (the launcher keeps the generic instantiation) and a
    success_timing='pre' env (plain): the same 30 steps through env.step
    against the oracle."""
    n = 64 * 3 + 5
    rng = np.random.RandomState(77 if variant == 'teleport' else 78)
    if variant == 'teleport':
        maze, kw, opts = 'teleport', {}, {}
    else:
        maze, kw, opts = 'large', dict(success_timing='pre'), dict(success_pre=1)
    sd, acts_np, far = _start(gpu, maze, n, False, rng, **kw)
    if variant == 'teleport':  # a third of the envs around the in-portals (maze.py:151-161)
        ins = np.array([[20.0, 12.0], [0.0, 16.0]])
        idx = np.flatnonzero(np.arange(n) % 3 == 0)
        idx = idx[idx != far]
        ang = rng.uniform(0, 2 * np.pi, len(idx))
        q = sd['qpos'].cpu().numpy()
        q[idx] = ins[idx % 2] + np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0, 2.2, len(idx))[:, None]
        sd['qpos'] = torch.tensor(q, device=gpu)
    env = _env(gpu, n, maze, **kw)
    env.reset(seed=SEED)
    env.load_state_dict(sd)
    outs, states = _bound_steps(env, torch.tensor(acts_np, device=gpu))
    ref, st = _oracle(maze, sd, acts_np, **opts)
    assert np.abs(np.stack([p['obs'] for p in outs]) - ref['obs']).max() <= TOL
    for key in ('terminated', 'truncated', 'success'):
        assert np.array_equal(np.stack([p[key] for p in outs]).astype(bool), ref[key].astype(bool)), key
    assert np.array_equal(np.stack([p['reward'] for p in outs]), ref['reward'])
    assert np.abs(states[-1]['qpos'] - st['qpos']).max() <= TOL
    assert np.array_equal(states[-1]['goal'], st['goal'])
    assert np.array_equal(states[-1]['episode'].view(np.uint32), st['episode'])
    assert ref['success'].sum() > 0 and ref['truncated'].sum() >= n
    if variant == 'success_pre':
        # 'pre' reads the position before the action: the far env is not at its goal at step 0
        assert ref['success'][0, far] == 0 and ref['success'][1, far] == 1
    else:
        outs_xy = np.array([[24.0, 0.0], [0.0, 20.0], [36.0, 20.0]])
        q_after = np.stack([s['qpos'] for s in states])
        assert (np.abs(q_after[:, :, None, :] - outs_xy).max(-1) == 0).any(-1).sum() > 0  # some env teleported
    env.close()


def test_success_threshold_at_the_last_bit(gpu):
    """The device's dist^2 <= goal_s2max test on distances within a few ulps of
    goal_tol = 1: zero actions in free space (the state is returned unchanged),
    goal at the origin, so dist^2 = fma(y, y, x * x) exactly as computed here
    with rationals; success must equal fl(sqrt(dist^2)) <= 1, and the sample
    holds squared distances in (1, goal_s2max] that a bare dist^2 <= tol^2
    would get wrong."""
    rng = np.random.RandomState(3)
    n = 4096
    ang = rng.uniform(0, 2 * np.pi, n)
    r = 1.0 + rng.randint(-6, 7, n) * 2.0 ** -53
    q = np.stack([np.cos(ang) * r, np.sin(ang) * r], 1)
    q[0], q[1], q[2] = [1.0, 0.0], [np.nextafter(1.0, 2.0), 0.0], [0.0, -np.nextafter(1.0, 2.0)]
    s = np.array([float(Fraction(y) * Fraction(y) + Fraction(float(np.float64(x) * np.float64(x))))
                  for x, y in q])
    want = np.sqrt(s) <= 1.0
    assert want[0] and not want[1] and not want[2]
    assert ((s > 1.0) & want).sum() > 20 and (~want).sum() > 500 and (s < 1.0).sum() > 500
    env = ogbench_amd.MazeEnv('point', 'large', num_envs=n, device=gpu, auto_reset=False)
    env.reset(seed=1, options=dict(task_id=1))
    sd = env.state_dict()
    sd['qpos'] = torch.tensor(q, device=gpu)  # cell (1, 1): centre (0, 0), walls 2 away
    sd['goal'] = torch.zeros(n, 2, dtype=torch.float64, device=gpu)
    env.load_state_dict(sd)
    ob, rew, term, trunc, info = env.step(torch.zeros(n, 2, device=gpu))
    assert np.array_equal(ob.cpu().numpy(), q)
    assert np.array_equal(info['success'].cpu().numpy().astype(bool), want)
    assert np.array_equal(term.cpu().numpy().astype(bool), want)
    env.close()
