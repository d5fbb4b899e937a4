"""On-device data collection (no host round trips per step): point mazes
(``collect_locomaze``) and powderworld play data (``collect_powderworld``, at
the end of this file).

Point mazes.

Batched counterpart of data_gen_scripts/generate_locomaze.py (hliuson/ogbench)
for the point agent, whose actor is the oracle subgoal direction (:44-46):
every step is one ``expert_action`` launch (BFS-table subgoal, normalised
direction, Gaussian action noise, clip) and one ``step`` launch; 'navigate'
resamples the goal of the envs that reached theirs (``set_goal``).  N envs run
their episodes in lock step (terminate_at_goal=False, so every episode lasts
max_episode_steps), and the result is laid out trajectory-major exactly like
the reference's saved arrays (observations / actions / qpos float32,
terminals bool).  qvel (info only) is not recorded.
"""

from __future__ import annotations

import numpy as np


def _torch():
    import torch

    return torch


def maze_cells(maze_map):
    """(all empty cells, vertex cells) as in generate_locomaze.py:62-90."""
    all_cells, vertex_cells = [], []
    m = maze_map
    for i in range(m.shape[0]):
        for j in range(m.shape[1]):
            if m[i, j] != 0:
                continue
            all_cells.append((i, j))
            if m[i - 1, j] == 0 and m[i + 1, j] == 0 and m[i, j - 1] == 1 and m[i, j + 1] == 1:
                continue
            if m[i, j - 1] == 0 and m[i, j + 1] == 0 and m[i - 1, j] == 1 and m[i + 1, j] == 1:
                continue
            vertex_cells.append((i, j))
    return np.array(all_cells, np.int32), np.array(vertex_cells, np.int32)


def collect_locomaze(env_name='pointmaze-large-v0', dataset_type='navigate', num_envs=1024, num_rounds=1,
                     max_episode_steps=1001, noise=0.2, seed=0, device=None):
    """Collect num_envs x num_rounds episodes of max_episode_steps transitions.

    Returns a dict of device tensors (trajectory-major): observations f32
    [E*T, 2], actions f32 [E*T, 2], terminals bool [E*T], qpos f32 [E*T, 2]."""
    torch = _torch()
    from .registry import make

    assert dataset_type in ('path', 'navigate'), 'point-maze collection supports path and navigate'
    env = make(env_name, num_envs=num_envs, device=device, terminate_at_goal=False,
               max_episode_steps=max_episode_steps, seed=seed)
    if env._loco_env_type != 'point':
        raise NotImplementedError('only the point agent has an oracle actor (ant/humanoid experts are SAC nets)')
    dev = env.device
    all_cells, vertex_cells = maze_cells(env.maze_map)
    all_t = torch.as_tensor(all_cells, device=dev)
    vert_t = torch.as_tensor(vertex_cells, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    T, N = int(max_episode_steps), int(num_envs)
    obs = torch.empty(num_rounds, T, N, 2, dtype=torch.float32, device=dev)
    act = torch.empty_like(obs)
    qpos = torch.empty_like(obs)
    term = torch.empty(num_rounds, T, N, dtype=torch.bool, device=dev)
    unit, off = env._maze_unit, env._offset_x
    for r in range(num_rounds):
        init_ij = all_t[torch.randint(len(all_t), (N,), device=dev, generator=gen)]
        goal_ij = vert_t[torch.randint(len(vert_t), (N,), device=dev, generator=gen)]
        task_xy = torch.stack([init_ij[:, 1] * unit - off, init_ij[:, 0] * unit - off,
                               goal_ij[:, 1] * unit - off, goal_ij[:, 0] * unit - off], 1).to(torch.float64)
        ob, _ = env.reset(seed=seed * 1000003 + r, options=dict(task_info=task_xy))
        for t in range(T):
            a = env.expert_action(noise=noise)
            obs[r, t] = ob
            qpos[r, t] = ob  # prev_qpos of a point agent is its observation
            act[r, t] = a
            ob, _, terminated, truncated, info = env.step(a)
            term[r, t] = terminated | truncated
            if dataset_type == 'navigate':
                new_ij = vert_t[torch.randint(len(vert_t), (N,), device=dev, generator=gen)]
                env.set_goal(new_ij, mask=info['success'])
    # [R, T, N, ...] -> trajectory-major [R, N, T, ...] -> rows
    def rows(x):
        x = x.permute(0, 2, 1, *range(3, x.dim())).contiguous()
        return x.reshape(num_rounds * N * T, *x.shape[3:])

    env.close()
    return dict(observations=rows(obs), actions=rows(act), terminals=rows(term), qpos=rows(qpos))


def _check_collect_args(num_envs, num_rounds, max_episode_steps, p_random_action, chunk):
    for name, v in (('num_envs', num_envs), ('num_rounds', num_rounds), ('max_episode_steps', max_episode_steps),
                    ('chunk', chunk)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
            raise ValueError(f'{name} must be a positive int, got {v!r}')
    if not 0.0 <= float(p_random_action) <= 1.0:
        raise ValueError(f'p_random_action must be in [0, 1], got {p_random_action}')


def collect_powderworld(env_name='powderworld-easy-v0', num_envs=1024, num_rounds=1, max_episode_steps=1001,
                        p_random_action=0.5, seed=0, device=None, chunk=48, tape=None, diagnostics=False):
    """Powderworld play data: num_envs x num_rounds episodes of max_episode_steps steps.

    Batched counterpart of data_gen_scripts/generate_powderworld.py
    (hliuson/ogbench) with the behaviours of ogbench/powderworld/behaviors.py.
    The play policy is open loop, so a round is: a data-collection reset
    (seed * 1000003 + r, the reseeding of collect_locomaze), ONE plan launch
    that writes every env's actions of the whole episode
    (include/ogbx_play.h), and the env's fused ``rollout`` in chunks of
    ``chunk`` steps; a chunk's [K, N, ...] block is transposed into the
    preallocated dataset by a torch copy.

    Returns a dict of device tensors laid out trajectory major like the
    reference's saved arrays, E = num_envs * num_rounds (episode r * num_envs +
    e is env e of round r), T = max_episode_steps:
      observations uint8 [E*T, H, W, 6]  row t of an episode is the observation
                                         BEFORE step t (row 0: the reset's)
      actions      int32 [E*T]
      terminals    bool  [E*T]           true at t == T - 1
    The reference's files store terminals as int32 (every key but the uint8
    observations goes through the `elif 'actions':` branch of
    generate_powderworld.py:99); load_dataset casts either to float32, so both
    load alike.  The script's train/val split is a slice the caller takes.

    tape: float64 [num_rounds, num_envs, L] of injected draws, for parity tests.
    diagnostics: also return 'used' int32 [E] (draws consumed per episode) and
    'decisions' int32 [E, (T + 2) // 3] (the plan's decision records)."""
    torch = _torch()
    from . import _play
    from .registry import make

    _check_collect_args(num_envs, num_rounds, max_episode_steps, p_random_action, chunk)
    if tape is not None and (np.ndim(tape) != 3 or tuple(np.shape(tape)[:2]) != (num_rounds, num_envs)):
        raise ValueError(f'tape must be [num_rounds={num_rounds}, num_envs={num_envs}, L], got {tuple(np.shape(tape))}')
    T, N, R = int(max_episode_steps), int(num_envs), int(num_rounds)
    env = make(env_name, num_envs=N, device=device, mode='data_collection', max_episode_steps=T, seed=seed)
    assert env._brush_size == env._grid_size, 'the behaviours assume brush_size == grid_size (behaviors.py:13)'
    dev, H = env.device, env._world_size
    obs = torch.empty(R, N, T, H, H, 6, dtype=torch.uint8, device=dev)
    act = torch.empty(R, N, T, dtype=torch.int32, device=dev)
    term = torch.empty(R, N, T, dtype=torch.bool, device=dev)
    used, dec = [], []
    out = None
    for r in range(R):
        round_seed = seed * 1000003 + r
        ob, _ = env.reset(seed=round_seed)
        plan = _play.plan(N, T, size=H // env._brush_size, num_elems=env._num_elems, xy_size=env._xy_action_size,
                          p_random_action=p_random_action, seed=round_seed, env_base=env.env_base,
                          tape=None if tape is None else tape[r], device=dev, records=diagnostics)
        a = plan['actions']
        act[r] = a.t()
        term[r] = plan['terminals'][None, :]
        obs[r, :, 0] = ob
        for t0 in range(0, T, chunk):
            k = min(chunk, T - t0)
            if out is None or out['obs'].shape[0] != k:
                out = None
            out = env.rollout(a[t0:t0 + k], out=out)
            keep = min(k, T - 1 - t0)  # the last step's observation opens no row
            if keep > 0:
                obs[r, :, t0 + 1:t0 + 1 + keep] = out['obs'][:keep].transpose(0, 1)
        if diagnostics:
            used.append(plan['used'])
            dec.append(plan['decisions'].t())
    env.close()
    data = dict(observations=obs.reshape(R * N * T, H, H, 6), actions=act.reshape(-1), terminals=term.reshape(-1))
    if diagnostics:
        data.update(used=torch.cat(used), decisions=torch.cat(dec))
    return data
