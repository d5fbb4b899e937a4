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

The fused path (``MazeEnv.collect``, include/ogbx_collect.h) runs the same
loop without the host in it: ``chunk`` steps per launch, every row written in
its final trajectory-major place.  It covers all four dataset kinds of the
script; 'stitch' (goal 4 BFS steps from the start, ``stitch_cells``) and
'explore' (a random direction every 10 steps) exist only there.
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


def stitch_cells(maze_map, adj_steps=4):
    """For every empty cell of maze_map (row-major, the order of maze_cells'
    all cells), the cells at BFS distance exactly adj_steps, in the discovery
    order of generate_locomaze.py:111-133 (neighbours (-1,0), (0,-1), (1,0),
    (0,1)): the goal candidates of a 'stitch' episode starting there.

    Returns (adj int32 [n_cells, max_count, 2] padded with -1, count int32
    [n_cells]).  A pure function of the map array."""
    m = np.asarray(maze_map)
    H, W = m.shape
    lists = []
    for i0 in range(H):
        for j0 in range(W):
            if m[i0, j0] != 0:
                continue
            dist = np.full((H, W), -1, np.int64)
            dist[i0, j0] = 0
            queue, adj = [(i0, j0)], []
            while queue:
                i, j = queue.pop(0)
                for di, dj in ((-1, 0), (0, -1), (1, 0), (0, 1)):
                    ni, nj = i + di, j + dj
                    if 0 <= ni < H and 0 <= nj < W and m[ni, nj] == 0 and dist[ni, nj] == -1:
                        dist[ni, nj] = dist[i, j] + 1
                        queue.append((ni, nj))
                        if dist[ni, nj] == adj_steps:
                            adj.append((ni, nj))
            lists.append(adj)
    count = np.array([len(a) for a in lists], np.int32)
    adj = np.full((len(lists), max(int(count.max()) if len(lists) else 0, 1), 2), -1, np.int32)
    for c, a in enumerate(lists):
        if a:
            adj[c, :len(a)] = a
    return adj, count


DATASET_TYPES = ('path', 'navigate', 'stitch', 'explore')


def _check_locomaze_args(dataset_type, num_envs, num_rounds, max_episode_steps, noise, fused, chunk, tape):
    """Argument checks of collect_locomaze, before any device is touched.
    Returns whether the fused path runs."""
    from . import _collect

    if dataset_type not in DATASET_TYPES:
        raise ValueError(f'dataset_type must be one of {DATASET_TYPES}, got {dataset_type!r}')
    for name, v in (('num_envs', num_envs), ('num_rounds', num_rounds), ('max_episode_steps', max_episode_steps),
                    ('chunk', chunk)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
            raise ValueError(f'{name} must be a positive int, got {v!r}')
    if not (isinstance(noise, (int, float, np.integer, np.floating)) and np.isfinite(noise) and noise >= 0):
        raise ValueError(f'noise must be a finite number >= 0, got {noise!r}')
    if fused not in (None, True, False):
        raise ValueError(f'fused must be None, True or False, got {fused!r}')
    if fused is None:
        fused = dataset_type in ('stitch', 'explore')
    if not fused and dataset_type in ('stitch', 'explore'):
        raise ValueError(f'{dataset_type!r} datasets are collected by the fused path only (fused=False given)')
    if tape is not None:
        if not fused:
            raise ValueError('a tape is taken by the fused path only')
        if not isinstance(tape, dict):
            raise ValueError('tape must be a dict of per-round draws ([num_rounds, ...] each)')
        for k, v in tape.items():
            if v is not None and (np.ndim(v) < 1 or np.shape(v)[0] != num_rounds):
                raise ValueError(f'tape[{k!r}] must have a leading dimension num_rounds = {num_rounds}')
        steps = _collect.check_tape({k: (None if v is None else v[0]) for k, v in tape.items()}, num_envs)
        if steps and steps < max_episode_steps:
            raise ValueError(f'the tape covers {steps} steps of {max_episode_steps}')
    return bool(fused)


def collect_locomaze(env_name='pointmaze-large-v0', dataset_type='navigate', num_envs=1024, num_rounds=1,
                     max_episode_steps=1001, noise=0.2, seed=0, device=None, fused=None, chunk=64, tape=None,
                     diagnostics=False):
    """Collect num_envs x num_rounds episodes of max_episode_steps transitions
    of a 'path', 'navigate', 'stitch' or 'explore' dataset
    (generate_locomaze.py:30-34).

    fused: None -- 'path' and 'navigate' run the stepwise launches (one
    expert_action, step and set_goal launch per step), 'stitch' and 'explore'
    the fused collector (``MazeEnv.collect``: ``chunk`` steps per launch, rows
    written in place); True -- the fused collector for any kind; False -- the
    stepwise launches ('path' / 'navigate' only).  The two paths draw from
    different Philox streams, so their datasets differ for one seed.
    tape (fused only): dict of injected draws, each [num_rounds, ...] of a
    ``MazeEnv.collect`` tape.

    Returns a dict of device tensors (trajectory-major): observations f32
    [E*T, 2], actions f32 [E*T, 2], terminals bool [E*T], qpos f32 [E*T, 2];
    with diagnostics (fused only) also init_ij and goal_ij int32 [E, 2], the
    cells every episode was reset with."""
    torch = _torch()
    from .registry import make

    fused = _check_locomaze_args(dataset_type, num_envs, num_rounds, max_episode_steps, noise, fused, chunk, tape)
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
    unit, off = env._maze_unit, env._offset_x
    if fused:
        R = int(num_rounds)
        data = dict(observations=torch.empty(R * N * T, 2, dtype=torch.float32, device=dev),
                    actions=torch.empty(R * N * T, 2, dtype=torch.float32, device=dev),
                    terminals=torch.empty(R * N * T, dtype=torch.bool, device=dev),
                    qpos=torch.empty(R * N * T, 2, dtype=torch.float32, device=dev))
        if dataset_type == 'stitch':
            adj, count = stitch_cells(env.maze_map)
            adj_t, count_t = torch.as_tensor(adj, device=dev), torch.as_tensor(count, device=dev).long()
        inits, goals = [], []
        for r in range(R):
            init_idx = torch.randint(len(all_t), (N,), device=dev, generator=gen)
            init_ij = all_t[init_idx]
            if dataset_type == 'stitch':
                # uniform over the cells 4 steps away; the start itself where there is none
                cnt = count_t[init_idx]
                pick = (torch.rand(N, dtype=torch.float64, device=dev, generator=gen) * cnt).long()
                pick = torch.minimum(pick, (cnt - 1).clamp(min=0))
                goal_ij = torch.where((cnt > 0)[:, None], adj_t[init_idx, pick], init_ij)
            else:
                goal_ij = vert_t[torch.randint(len(vert_t), (N,), device=dev, generator=gen)]
            task_xy = torch.stack([init_ij[:, 1] * unit - off, init_ij[:, 0] * unit - off,
                                   goal_ij[:, 1] * unit - off, goal_ij[:, 0] * unit - off], 1).to(torch.float64)
            round_seed = seed * 1000003 + r
            env.reset(seed=round_seed, options=dict(task_info=task_xy))
            out = dict(data, row_offset=r * N * T, row_stride=T)
            tape_r = None if tape is None else {k: (None if v is None else v[r]) for k, v in tape.items()}
            for t0 in range(0, T, chunk):
                env.collect(min(chunk, T - t0), out, dataset_type, noise=noise, goal_cells=vert_t, tape=tape_r,
                            seed=round_seed)
            inits.append(init_ij)
            goals.append(goal_ij)
        if diagnostics:
            data.update(init_ij=torch.cat(inits).to(torch.int32), goal_ij=torch.cat(goals).to(torch.int32))
        env.close()
        return data
    obs = torch.empty(num_rounds, T, N, 2, dtype=torch.float32, device=dev)
    act = torch.empty_like(obs)
    qpos = torch.empty_like(obs)
    term = torch.empty(num_rounds, T, N, dtype=torch.bool, device=dev)
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
