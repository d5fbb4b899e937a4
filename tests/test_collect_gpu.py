"""GPU: the fused point-maze collector (maze_collect_kernel through
MazeEnv.collect / datagen.collect_locomaze) against the stepwise launches it
fuses (bit for bit), against the CPU restatement of the script on the oracle
(tests/collect_np.py, teacher-forced), and its Philox streams against the
counter layout documented in include/ogbx_collect.h.

Shapes: N = 70 envs (two waves, the second partial), T = 25 steps, chunks of 7
(divides neither T nor the explore period of 10: a direction crosses a chunk
boundary and the last chunk is short)."""

import numpy as np
import pytest
import torch

import collect_np
import ogbench_amd
from ogbench_amd.datagen import collect_locomaze, maze_cells, stitch_cells
from oracle import locomaze as orc
from test_locomaze_gpu import TOL

pytestmark = pytest.mark.gpu

N, T, CHUNK = 70, 25, 7
MEDIUM, TELEPORT = 'pointmaze-medium-v0', 'pointmaze-teleport-v0'
MODES = ('path', 'navigate', 'stitch', 'explore')
TP_IN = ((4, 6), (5, 1))  # the teleport maze's in-portal cells (maze.py:151-161)


def _inputs(env_name, mode, seed, n=N):
    """Start states and a full tape for one round of `mode`."""
    rng = np.random.RandomState(1000 * seed + MODES.index(mode))
    mp, _ = orc.tables(collect_np.maze_name(env_name))
    all_cells, vert = (np.array(c, np.int32) for c in collect_np.cells_of(mp))
    init = all_cells[rng.randint(len(all_cells), size=n)]
    noise = rng.uniform(-1, 1, (n, 4))
    if mode == 'navigate':
        # goal cell = init cell, no goal noise at reset: goals are reached within the episode
        goal = init.copy()
        noise[:, 2:] = 0.0
    elif mode == 'stitch':
        adj, count = stitch_cells(mp)
        index = {tuple(c): k for k, c in enumerate(all_cells.tolist())}
        goal = np.array([adj[index[tuple(c)], rng.randint(count[index[tuple(c)]])] if count[index[tuple(c)]] else c
                         for c in init.tolist()], np.int32)
    else:
        goal = vert[rng.randint(len(vert), size=n)]
    if env_name == TELEPORT:
        init[: n // 3] = np.array(TP_IN)[rng.randint(2, size=n // 3)]  # some envs start inside an in-portal cell
    task_xy = np.concatenate([collect_np.ij_to_xy(init), collect_np.ij_to_xy(goal)], 1)
    tape = dict(normal=rng.normal(0, 0.2, (T, n, 2)), goal_pick=rng.randint(len(vert), size=(T, n)).astype(np.int32),
                goal_noise=rng.uniform(-1, 1, (T, n, 2)), dir=rng.randn(-(-T // collect_np.PERIOD), n, 2))
    return dict(task_xy=task_xy, noise=noise, tape=tape, vert=vert, maze=collect_np.maze_name(env_name))


def _env(gpu, env_name, inp, n=N, seed=11, **kw):
    env = ogbench_amd.make(env_name, num_envs=n, device=gpu, terminate_at_goal=False, max_episode_steps=T, **kw)
    env.reset(seed=seed, options=dict(task_info=torch.tensor(inp['task_xy']), noise=torch.tensor(inp['noise'])))
    return env


def _columns(gpu, n=N, rows=None):
    rows = n * T if rows is None else rows
    return dict(observations=torch.full((rows, 2), np.nan, dtype=torch.float32, device=gpu),
                actions=torch.full((rows, 2), np.nan, dtype=torch.float32, device=gpu),
                terminals=torch.zeros(rows, dtype=torch.bool, device=gpu),
                qpos=torch.full((rows, 2), np.nan, dtype=torch.float32, device=gpu))


def _fused(env, gpu, mode, inp, chunk=CHUNK, tape=True, seed=None, diagnostics=False, n=N, drop=()):
    """One round through MazeEnv.collect in chunks; returns (columns, diagnostics over the episode)."""
    out = _columns(gpu, n)
    tp = None
    if tape:
        tp = {k: torch.tensor(v) for k, v in inp['tape'].items() if k not in drop}
    diags = []
    for t0 in range(0, T, chunk):
        diags.append(env.collect(min(chunk, T - t0), out, mode, noise=0.2, goal_cells=torch.tensor(inp['vert']),
                                 tape=tp, seed=seed, diagnostics=diagnostics))
    cols = {k: v.cpu().numpy() for k, v in out.items()}
    diag = {k: torch.cat([d[k] for d in diags]).cpu().numpy() for k in diags[0]} if diagnostics else {}
    return cols, diag


def _stepwise(env, gpu, mode, inp):
    """The launches the collector fuses, driven from the host with the tape's draws."""
    tape, vert = inp['tape'], torch.tensor(inp['vert'], device=gpu)
    obs = np.empty((T, N, 2), np.float32)
    act = np.empty((T, N, 2), np.float32)
    term = np.empty((T, N), bool)
    succ = np.empty((T, N), bool)
    if mode == 'explore':
        ex = collect_np.explore_actions(tape['dir'], tape['normal'])
    for t in range(T):
        obs[t] = env.get_xy().to(torch.float32).cpu().numpy()
        if mode == 'explore':
            a = torch.tensor(ex[t], dtype=torch.float64, device=gpu)
        else:
            a = env.expert_action(noise=0.2, normal=torch.tensor(tape['normal'][t]))
        act[t] = a.to(torch.float32).cpu().numpy()
        _, _, terminated, truncated, info = env.step(a)
        term[t] = (terminated | truncated).cpu().numpy()
        succ[t] = info['success'].cpu().numpy()
        if mode == 'navigate':
            env.set_goal(vert[torch.tensor(tape['goal_pick'][t].astype(np.int64), device=gpu)], mask=info['success'],
                         noise=torch.tensor(tape['goal_noise'][t]))
    rows = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape(N * T, *x.shape[2:])
    return dict(observations=rows(obs), actions=rows(act), terminals=rows(term), qpos=rows(obs)), succ


def _state(env):
    q, g, e, _, _ = env._state_views()
    return q.cpu().numpy().copy(), g.cpu().numpy().copy(), e.cpu().numpy().copy()


def _assert_same_run(env_name, gpu, mode, inp, drop=()):
    a, b = _env(gpu, env_name, inp), _env(gpu, env_name, inp)
    fused, _ = _fused(a, gpu, mode, inp, drop=drop)
    step, succ = _stepwise(b, gpu, mode, inp)
    for k in ('observations', 'actions', 'terminals', 'qpos'):
        assert not np.isnan(fused[k].astype(np.float64)).any(), k
        assert np.array_equal(fused[k], step[k]), (mode, k)
    for x, y, name in zip(_state(a), _state(b), ('qpos', 'goal', 'elapsed')):
        assert np.array_equal(x, y), (mode, name)
    assert (_state(a)[2] == T).all()
    a.close()
    b.close()
    return fused, succ


@pytest.mark.parametrize('mode', MODES)
def test_fused_equals_stepwise_bit_for_bit(gpu, mode):
    inp = _inputs(MEDIUM, mode, seed=0)
    fused, succ = _assert_same_run(MEDIUM, gpu, mode, inp)
    assert np.array_equal(np.nonzero(fused['terminals'])[0], np.arange(T - 1, N * T, T))
    if mode == 'navigate':
        # envs that resample a goal at least once: without them the test proves nothing about step 5
        assert succ.any(0).sum() >= N / 4


@pytest.mark.parametrize('mode', MODES)
def test_fused_against_the_cpu_restatement_teacher_forced(gpu, mode):
    inp = _inputs(MEDIUM, mode, seed=1)
    env = _env(gpu, MEDIUM, inp)
    cols, diag = _fused(env, gpu, mode, inp, diagnostics=True)
    q_end, g_end, _ = _state(env)
    env.close()
    tape, maze = inp['tape'], inp['maze']
    q, g, succ = diag['qpos64'], diag['goal64'], diag['success']
    assert q.shape == g.shape == (T, N, 2) and succ.shape == (T, N) and succ.dtype == np.bool_
    q_next = np.concatenate([q[1:], q_end[None]])
    g_next = np.concatenate([g[1:], g_end[None]])
    qf, gf, zf = q.reshape(-1, 2), g.reshape(-1, 2), tape['normal'].reshape(-1, 2)
    # the action of every row, exactly
    if mode == 'explore':
        want_a = collect_np.explore_actions(tape['dir'], tape['normal']).reshape(-1, 2)
    else:
        want_a = orc.expert_action(maze, qf, gf, zf)
    rows = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape(N * T, *x.shape[2:])
    assert np.array_equal(cols['actions'], rows(want_a.reshape(T, N, 2)).astype(np.float32))
    assert np.array_equal(cols['observations'], rows(q).astype(np.float32))
    assert np.array_equal(cols['qpos'], cols['observations'])
    # the next state: exact in free space, within the contact tolerance otherwise
    ref, contact = orc.physics(maze, qf, want_a, nthreads=8)
    got = q_next.reshape(-1, 2)
    free = contact == 0
    assert np.array_equal(got[free], ref[free])
    assert np.abs(got - ref).max() <= TOL
    if mode == 'explore':
        assert contact.mean() >= 0.05  # contact rows by the oracle's flag
    # success flags (post timing, on the state the step reached) and the new goals
    want_s = collect_np.success_of(got, gf).reshape(T, N)
    assert np.array_equal(succ, want_s)
    want_g = g.copy()
    if mode == 'navigate':
        fresh = collect_np.new_goals(inp['vert'], tape['goal_pick'], tape['goal_noise'])
        want_g = np.where(want_s[..., None], fresh, g)
        assert want_s.any(0).sum() >= N / 4
    assert np.array_equal(g_next, want_g)


def test_teleport_maze_explore_equals_stepwise(gpu):
    """No teleport tape: both paths draw the out-portal from the step's own stream."""
    inp = _inputs(TELEPORT, 'explore', seed=2)
    fused, _ = _assert_same_run(TELEPORT, gpu, 'explore', inp)
    o = fused['observations'].reshape(N, T, 2)
    jumps = np.abs(np.diff(o, axis=1)).max(-1) > 1.0
    assert jumps.sum() >= 1


def _philox_run(gpu, mode, inp, chunk, seed, n=N, env_base=0, sl=slice(None)):
    sub = dict(inp, task_xy=inp['task_xy'][sl], noise=inp['noise'][sl])
    env = _env(gpu, MEDIUM, sub, n=n, env_base=env_base)
    cols, diag = _fused(env, gpu, mode, sub, chunk=chunk, tape=False, seed=seed, diagnostics=True, n=n)
    env.close()
    return cols, diag


@pytest.mark.parametrize('mode', ['navigate', 'explore'])
def test_philox_streams_do_not_depend_on_chunks_or_batch(gpu, mode):
    inp = _inputs(MEDIUM, mode, seed=3)
    base, _ = _philox_run(gpu, mode, inp, CHUNK, seed=5)
    for chunk in (1, T):
        other, _ = _philox_run(gpu, mode, inp, chunk, seed=5)
        for k in base:
            assert np.array_equal(base[k], other[k]), (chunk, k)
    part, _ = _philox_run(gpu, mode, inp, CHUNK, seed=5, n=3, env_base=5, sl=slice(5, 8))
    head, _ = _philox_run(gpu, mode, inp, CHUNK, seed=5, n=8, sl=slice(0, 8))
    again, _ = _philox_run(gpu, mode, inp, CHUNK, seed=5)
    reseeded, _ = _philox_run(gpu, mode, inp, CHUNK, seed=6)
    for k in base:
        assert np.array_equal(part[k], base[k][5 * T:8 * T]), k
        assert np.array_equal(head[k], base[k][:8 * T]), k
        assert np.array_equal(again[k], base[k]), k
    assert not np.array_equal(reseeded['actions'], base['actions'])


def test_philox_goal_draws_follow_the_documented_layout(gpu):
    inp = _inputs(MEDIUM, 'navigate', seed=4)
    env_base, seed = 1 << 33, (7 << 40) + 12345  # both halves of the env index and of the seed in play
    env = _env(gpu, MEDIUM, inp, env_base=env_base)
    _, diag = _fused(env, gpu, 'navigate', inp, tape=False, seed=seed, diagnostics=True)
    _, g_end, _ = _state(env)
    env.close()
    g_next = np.concatenate([diag['goal64'][1:], g_end[None]])
    succ = diag['success']
    assert succ.any(0).sum() >= N / 4
    for t, e in zip(*np.nonzero(succ)):
        pick = collect_np.goal_pick(seed, env_base + int(e), int(t), len(inp['vert']))
        r = collect_np.goal_noise(seed, env_base + int(e), int(t))
        want = collect_np.new_goals(inp['vert'], pick, np.array(r))
        assert np.array_equal(g_next[t, e], want), (t, e)


def test_philox_action_noise(gpu):
    """The action noise of Philox mode: its moments on the unclipped rows, and every action against the
    draw recomputed on the CPU from the documented counter layout.

    Keeping only unclipped rows truncates the noise (a direction component near +-1 keeps only the
    draws that point inward), so about 2,000 of the 3,500 samples remain and their pooled standard
    deviation sits slightly below 0.2: a CPU run of this case on the oracle gave mean 0.0019 and
    standard deviation 0.1896 at 2,034 samples."""
    inp = _inputs(MEDIUM, 'path', seed=5)
    seed = 9
    cols, diag = _philox_run(gpu, 'path', inp, CHUNK, seed=seed)
    q, g = diag['qpos64'].reshape(-1, 2), diag['goal64'].reshape(-1, 2)
    clean = orc.expert_action(inp['maze'], q, g, np.zeros_like(q))
    rows = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape(N * T, *x.shape[2:])
    a = cols['actions'].astype(np.float64)
    keep = (np.abs(a) < 1.0).all(1)  # rows where neither component is clipped
    d = (a - rows(clean.reshape(T, N, 2)))[keep]
    print('unclipped samples', d.size, 'mean', d.mean(), 'std', d.std())
    assert abs(d.mean()) <= 0.012 and abs(d.std() - 0.2) <= 0.012
    # every action: clip(direction + z) with z from the layout; 2e-7 covers the float32 rounding of the
    # row (6e-8 at 1) and the last-place differences of log / cos / sin between the device and libm
    z = np.array([[collect_np.action_normal(seed, e, t, 0.2) for e in range(N)] for t in range(T)])
    want = orc.expert_action(inp['maze'], q, g, z.reshape(-1, 2))
    assert np.abs(a - rows(want.reshape(T, N, 2))).max() <= 2e-7


def test_philox_explore_directions_follow_the_documented_layout(gpu):
    inp = _inputs(MEDIUM, 'explore', seed=5)
    seed = 9
    cols, _ = _philox_run(gpu, 'explore', inp, CHUNK, seed=seed)
    periods = -(-T // collect_np.PERIOD)
    d = np.array([[collect_np.explore_normal(seed, e, p) for e in range(N)] for p in range(periods)])
    z = np.array([[collect_np.action_normal(seed, e, t, 0.2) for e in range(N)] for t in range(T)])
    want = collect_np.explore_actions(d, z)
    rows = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape(N * T, *x.shape[2:])
    assert np.abs(cols['actions'].astype(np.float64) - rows(want)).max() <= 2e-7


@pytest.mark.parametrize('kind, env_name', [('stitch', MEDIUM), ('explore', MEDIUM), ('stitch', TELEPORT)])
def test_collect_locomaze_stitch_and_explore(gpu, kind, env_name):
    R = 2
    d = collect_locomaze(env_name, kind, num_envs=N, num_rounds=R, max_episode_steps=T, seed=3, device=gpu,
                         chunk=CHUNK, diagnostics=True)
    E = R * N
    assert d['observations'].shape == d['actions'].shape == d['qpos'].shape == (E * T, 2)
    assert d['observations'].dtype == d['actions'].dtype == d['qpos'].dtype == torch.float32
    assert d['terminals'].shape == (E * T,) and d['terminals'].dtype == torch.bool
    assert np.array_equal(np.nonzero(d['terminals'].cpu().numpy())[0], np.arange(T - 1, E * T, T))
    act = d['actions'].cpu().numpy()
    assert np.isfinite(act).all() and np.abs(act).max() <= 1.0
    assert torch.equal(d['observations'], d['qpos'])
    init, goal = d['init_ij'].cpu().numpy(), d['goal_ij'].cpu().numpy()
    assert init.shape == goal.shape == (E, 2)
    mp, _ = orc.tables(collect_np.maze_name(env_name))
    # every episode starts in its init cell (reset noise is at most a quarter cell)
    o0 = d['observations'].cpu().numpy().reshape(E, T, 2)[:, 0]
    assert np.abs(o0 - collect_np.ij_to_xy(init)).max() <= 1.0
    if kind == 'stitch':
        fallback = 0
        for c, gcell in zip(init.tolist(), goal.tolist()):
            want = collect_np.script_adj_cells(mp, tuple(c))
            if want:
                assert tuple(gcell) in want
            else:
                assert gcell == c
                fallback += 1
        lonely = [c for c in collect_np.cells_of(mp)[0] if not collect_np.script_adj_cells(mp, c)]
        assert len(lonely) == (1 if env_name == TELEPORT else 0)
        assert fallback == sum(tuple(c) == lonely[0] for c in init.tolist()) if lonely else fallback == 0
        if env_name == MEDIUM:
            assert len({tuple(x) for x in goal.tolist()}) > 5  # the draw spreads over the candidates


def test_collect_locomaze_navigate_fused_and_default(gpu):
    n, t = 64, 120  # the shapes of test_expert_gpu.test_collect_navigate
    d = collect_locomaze(MEDIUM, 'navigate', num_envs=n, max_episode_steps=t, noise=0.2, seed=1, device=gpu,
                         fused=True)
    obs, act, term = d['observations'].cpu().numpy(), d['actions'].cpu().numpy(), d['terminals'].cpu().numpy()
    assert obs.shape == (n * t, 2) and obs.dtype == np.float32 and term.dtype == np.bool_
    assert np.array_equal(np.nonzero(term)[0], np.arange(t - 1, n * t, t))
    assert np.abs(act).max() <= 1.0
    assert np.abs(np.diff(obs.reshape(n, t, 2), axis=1)).max() < 0.5
    # the default is the stepwise path, unchanged: the same tensors as fused=False
    kw = dict(num_envs=n, max_episode_steps=30, noise=0.2, seed=1, device=gpu)
    default, stepwise = collect_locomaze(MEDIUM, 'navigate', **kw), collect_locomaze(MEDIUM, 'navigate', fused=False, **kw)
    assert set(default) == {'observations', 'actions', 'terminals', 'qpos'}
    for k in default:
        assert torch.equal(default[k], stepwise[k]), k
    assert not torch.equal(default['actions'], d['actions'][:default['actions'].shape[0]])


def test_collect_refusals(gpu):
    import ctypes

    from ogbench_amd import _collect, _lib

    inp = _inputs(MEDIUM, 'path', seed=6)
    cells = torch.tensor(inp['vert'])
    # an env that terminates at its goal
    env = ogbench_amd.make(MEDIUM, num_envs=N, device=gpu, max_episode_steps=T)
    env.reset(seed=0)
    with pytest.raises(ValueError, match='terminate_at_goal'):
        env.collect(1, _columns(gpu), 'path')
    L = _collect.bind()
    cols = _columns(gpu)
    cfg = _collect.CollectConfig(mode=0, explore_period=10, noise=0.2)
    o = _collect.CollectOutputs(row_stride=T, row_offset=0, **{k: cols[k].data_ptr() for k in _collect.COLUMNS})
    assert L.ogbx_maze_collect(env._h, cfg, None, 0, 1, 0, o, None) == _lib.OGBX_EINVAL
    assert 'terminate_at_goal' in _lib.last_error()
    env.close()
    # an ant handle
    ant = ogbench_amd.make('antmaze-medium-v0', num_envs=4, device=gpu, terminate_at_goal=False, max_episode_steps=T)
    with pytest.raises(ValueError, match='point'):
        ant.collect(1, _columns(gpu, 4), 'path')
    assert L.ogbx_maze_collect(ant._h, cfg, None, 0, 1, 0, o, None) == _lib.OGBX_EINVAL
    assert 'point' in _lib.last_error()
    ant.close()
    env = _env(gpu, MEDIUM, inp)
    before = _state(env)
    # a null required output, k_steps <= 0 (the C call itself)
    bad = _collect.CollectOutputs(row_stride=T, row_offset=0, observations=cols['observations'].data_ptr())
    assert L.ogbx_maze_collect(env._h, cfg, None, 0, 1, 0, bad, None) == _lib.OGBX_EINVAL
    assert L.ogbx_maze_collect(env._h, cfg, None, 0, 0, 0, o, None) == _lib.OGBX_EINVAL
    assert L.ogbx_maze_collect(env._h, cfg, None, T, 1, 0, o, None) == _lib.OGBX_EINVAL
    assert 'time limit' in _lib.last_error()
    with pytest.raises(ValueError, match='k_steps'):
        env.collect(0, cols, 'path')
    # a chunk past the time limit, at the start and after some steps
    with pytest.raises(ValueError, match='time limit'):
        env.collect(T + 1, cols, 'path')
    env.collect(T - 3, cols, 'path')
    with pytest.raises(ValueError, match='time limit'):
        env.collect(4, cols, 'path')
    env.collect(3, cols, 'path')
    assert (_state(env)[2] == T).all()
    env.reset(seed=11, options=dict(task_info=torch.tensor(inp['task_xy']), noise=torch.tensor(inp['noise'])))
    for x, y in zip(_state(env), before):
        assert np.array_equal(x, y)
    # tapes of the wrong shape
    for tape in (dict(normal=torch.zeros(T, N - 1, 2)), dict(normal=torch.zeros(T, N)),
                 dict(goal_pick=torch.zeros(T, N, 2, dtype=torch.int32)), dict(dir=torch.zeros(3, N, 3)),
                 dict(normal=torch.zeros(T, N, 2), dir=torch.zeros(2, N, 2)), dict(normal=torch.zeros(5, N, 2))):
        with pytest.raises(ValueError, match='tape'):
            env.collect(CHUNK, cols, 'navigate', goal_cells=cells, tape=tape)
    # columns that do not hold the rows, a mode that does not exist, navigate without cells
    with pytest.raises(ValueError, match='rows'):
        env.collect(CHUNK, _columns(gpu, rows=N * T - 1), 'path')
    with pytest.raises(ValueError, match='mode'):
        env.collect(CHUNK, cols, 'wander')
    with pytest.raises(ValueError, match='goal_cells'):
        env.collect(CHUNK, cols, 'navigate')
    # nothing above moved the envs
    for x, y in zip(_state(env), before):
        assert np.array_equal(x, y)
    env.close()
