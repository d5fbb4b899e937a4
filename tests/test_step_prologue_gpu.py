"""The plain step's prologue and epilogue (maze_step_kernel<.., kPlain>: the
wall-mask table per wave with no block barrier, every load unconditional with
lanes past the last env reading through a clamped index, the epilogue's
arguments reloaded from the kernarg segment) against the generic
instantiation, which keeps the block-shared table and the predicated loads:
ogbx_maze_set_envs_per_wave(h, 32) + ogbx_maze_step(k_steps = 1).  Outputs and
state bit for bit over 12 steps with TimeLimit auto-resets inside them, f32
and f64 actions.

Shapes: N = 255, 257 and 321 -- a block whose waves 1-3 have no env, a wave
with one env, lanes that load through the clamp; outputs are slices of larger
sentinel-filled buffers whose margins must survive.  Maze 'giant' (192 cells:
table entries >= 128 are the upper half of each lane's 8-byte piece) and
'arena'.  Envs that start inside a wall cell or off the map read the wave's
table through point_step_walled's generic pointer.  Two handles of different
mazes stepping alternately on one stream must each equal their solo run (no
table of an earlier launch survives in LDS).
"""
import numpy as np
import pytest
import torch

import ogbench_amd
from ogbench_amd import _lib
from oracle import locomaze as orc

pytestmark = pytest.mark.gpu
TOL = 1e-9  # contact dynamics against the oracle, as tests/test_locomaze_gpu.py
K, MAX_STEPS, SEED = 12, 5, 9
PAD = 64  # margin rows on both sides of every output
SENT_F, SENT_B = -7.0, 0xA5
OUT_KEYS = ('obs', 'reward', 'terminated', 'truncated', 'success', 'final_obs')
STATE_KEYS = ('qpos', 'goal', 'elapsed', 'task', 'episode')


def _env(gpu, n, maze):
    return ogbench_amd.MazeEnv('point', maze, num_envs=n, device=gpu, auto_reset=True, max_episode_steps=MAX_STEPS)


def _start(gpu, maze, n, f64, rng, walled=False):
    """Start state (within 1.9 of cell centres; every third env in a cell of
    the upper half of the table) and K actions.  walled: envs 0..4 inside wall cells
    (two of them of the map's upper half), env n - 1 off the map."""
    env = _env(gpu, n, maze)
    tid = torch.tensor((np.arange(n) % env.num_tasks + 1).astype(np.int32))
    env.reset(seed=SEED, options=dict(task_id=tid))
    sd = env.state_dict()
    env.close()
    mp, _ = orc.tables(maze)
    H, W = mp.shape
    free = np.argwhere(mp == 0)
    half = 128 if H * W > 128 else H * W // 2  # 'giant': the upper half of each lane's 8-byte piece of the table
    high = free[free[:, 0] * W + free[:, 1] >= half]
    c = free[rng.randint(len(free), size=n)]
    third = np.arange(n) % 3 == 0
    c[third] = high[rng.randint(len(high), size=int(third.sum()))]
    off = rng.uniform(-1.9, 1.9, (n, 2))
    if walled:
        walls = np.argwhere(mp == 1)
        inner = walls[(walls[:, 0] > 0) & (walls[:, 0] < H - 1) & (walls[:, 1] > 0) & (walls[:, 1] < W - 1)]
        hi_in = inner[inner[:, 0] * W + inner[:, 1] >= half]
        c[0:2] = hi_in[rng.randint(len(hi_in), size=2)]
        c[2:4] = inner[rng.randint(len(inner), size=2)]
        c[4] = walls[0]  # the map's corner cell
        off[0:5] = rng.uniform(-1.5, 1.5, (5, 2))
    q = np.stack([c[:, 1] * 4.0 - 4.0 + off[:, 1], c[:, 0] * 4.0 - 4.0 + off[:, 0]], 1)
    if walled:
        q[n - 1] = [-13.0, 5.0]
    acts = rng.uniform(-1, 1, (K, n, 2)).astype(np.float64 if f64 else np.float32)
    sd['qpos'] = torch.tensor(q, device=gpu)
    sd['elapsed'] = torch.full((n,), MAX_STEPS - 3, dtype=torch.int32, device=gpu)
    return sd, acts, c


def _loaded(gpu, n, maze, sd):
    env = _env(gpu, n, maze)
    env.reset(seed=SEED)
    env.load_state_dict(sd)
    return env


def _state(env):
    sd = env.state_dict()
    return {k: sd[k].cpu().numpy() for k in STATE_KEYS}


class _Outputs:
    """Step outputs as the middle n rows of sentinel-filled buffers."""

    def __init__(self, n, dev):
        m = n + 2 * PAD
        self.n = n
        self.big = dict(obs=torch.full((m, 2), SENT_F, dtype=torch.float64, device=dev),
                        reward=torch.full((m,), SENT_F, dtype=torch.float32, device=dev),
                        terminated=torch.full((m,), SENT_B, dtype=torch.uint8, device=dev),
                        truncated=torch.full((m,), SENT_B, dtype=torch.uint8, device=dev),
                        success=torch.full((m,), SENT_B, dtype=torch.uint8, device=dev),
                        final_obs=torch.full((m, 2), SENT_F, dtype=torch.float64, device=dev))
        self.mid = {k: v[PAD:PAD + n] for k, v in self.big.items()}

    def ptrs(self):
        return [_lib.ptr(self.mid[k]) for k in OUT_KEYS]

    def take(self):
        """The n rows of this step; the margins must hold their sentinels."""
        for k, v in self.big.items():
            a = v.cpu().numpy()
            sent = SENT_B if a.dtype == np.uint8 else SENT_F
            assert (a[:PAD] == sent).all() and (a[PAD + self.n:] == sent).all(), k
        return {k: v.cpu().numpy().copy() for k, v in self.mid.items()}


def _plain_steps(env, acts):
    """K single steps through ogbx_maze_bind_step + ogbx_maze_step_bound (env.step's launch)."""
    out = _Outputs(env.num_envs, env.device)
    _lib.check(env._L.ogbx_maze_bind_step(env._h, *out.ptrs(), 1))
    outs, states = [], []
    for t in range(K):
        out.mid['final_obs'].fill_(SENT_F)
        a = acts[t].contiguous()
        _lib.check(env._L.ogbx_maze_step_bound(env._h, _lib.ptr(a), int(a.dtype == torch.float64), env._stream()))
        outs.append(out.take())
        states.append(_state(env))
    return outs, states


def _generic_steps(env, acts):
    """The same steps through the generic instantiation: 32 envs per wave, ogbx_maze_step with k_steps = 1."""
    _lib.check(env._L.ogbx_maze_set_envs_per_wave(env._h, 32))
    out = _Outputs(env.num_envs, env.device)
    outs, states = [], []
    for t in range(K):
        out.mid['final_obs'].fill_(SENT_F)
        a = acts[t].contiguous()
        _lib.check(env._L.ogbx_maze_step(env._h, _lib.ptr(a), int(a.dtype == torch.float64), 1, *out.ptrs(), 1,
                                         env._stream()))
        outs.append(out.take())
        states.append(_state(env))
    return outs, states


def _oracle(maze, sd, acts):
    st = dict(qpos=sd['qpos'].cpu().numpy().copy(), goal=sd['goal'].cpu().numpy().copy(),
              elapsed=sd['elapsed'].cpu().numpy().copy(), task=sd['task'].cpu().numpy().copy(),
              episode=sd['episode'].cpu().numpy().view(np.uint32).copy(), opts=orc._opts(max_steps=MAX_STEPS))
    return orc.step(maze, st, acts, auto_reset=1, key=orc.philox_key(SEED, orc.TAG_MAZE_RESET)), st


def _assert_same(plain, plain_states, gen, gen_states):
    for t in range(K):
        for key in OUT_KEYS:
            assert plain[t][key].dtype == gen[t][key].dtype
            assert np.array_equal(plain[t][key].view(np.uint8), gen[t][key].view(np.uint8)), (key, t)
        for key in STATE_KEYS:
            assert np.array_equal(plain_states[t][key].view(np.uint8), gen_states[t][key].view(np.uint8)), (key, t)


def _assert_oracle(maze, sd, acts_np, plain, plain_states):
    ref, st = _oracle(maze, sd, acts_np)
    assert np.abs(np.stack([p['obs'] for p in plain]) - ref['obs']).max() <= TOL
    for key in ('terminated', 'truncated', 'success'):
        assert np.array_equal(np.stack([p[key] for p in plain]).astype(bool), ref[key].astype(bool)), key
    assert np.array_equal(np.stack([p['reward'] for p in plain]), ref['reward'])
    assert np.abs(plain_states[-1]['qpos'] - st['qpos']).max() <= TOL
    assert np.array_equal(plain_states[-1]['episode'].view(np.uint32), st['episode'])
    # the TimeLimit ends every episode still running at step 2 (auto-resets inside the K steps)
    running = ~ref['terminated'][:3].astype(bool).any(0)
    assert ref['truncated'][2][running].all() and running.sum() * 2 > acts_np.shape[1]
    ended = (ref['terminated'] | ref['truncated']).astype(bool)
    fin = np.stack([p['final_obs'] for p in plain])
    assert (fin[~ended] == SENT_F).all() and (fin[ended] != SENT_F).all()
    return ref


@pytest.mark.parametrize('n', [255, 257, 321])
@pytest.mark.parametrize('f64', [False, True])
@pytest.mark.parametrize('maze', ['giant', 'arena'])
def test_prologue_equals_generic(gpu, maze, f64, n):
    rng = np.random.RandomState(1000 * n + 2 * sum(map(ord, maze)) + int(f64))
    sd, acts_np, cells = _start(gpu, maze, n, f64, rng)
    mp, _ = orc.tables(maze)
    if maze == 'giant':
        assert mp.size == 192 and (cells[:, 0] * mp.shape[1] + cells[:, 1] >= 128).sum() * 4 >= n
    # some envs start in contact (their waves run the lean loop, some lanes bail to the full one)
    _, contact = orc.physics(maze, sd['qpos'].cpu().numpy(), acts_np[0])
    assert contact.sum() >= 4
    acts = torch.tensor(acts_np, device=gpu)
    e_plain, e_gen = _loaded(gpu, n, maze, sd), _loaded(gpu, n, maze, sd)
    plain, plain_states = _plain_steps(e_plain, acts)
    gen, gen_states = _generic_steps(e_gen, acts)
    _assert_same(plain, plain_states, gen, gen_states)
    _assert_oracle(maze, sd, acts_np, plain, plain_states)
    e_plain.close()
    e_gen.close()


@pytest.mark.parametrize('f64', [False, True])
def test_table_through_generic_pointer(gpu, f64):
    """Envs inside wall cells and one off the map: point_step_walled reads the
    wave's table through its generic pointer."""
    maze, n = 'giant', 257
    rng = np.random.RandomState(41 + int(f64))
    sd, acts_np, cells = _start(gpu, maze, n, f64, rng, walled=True)
    mp, _ = orc.tables(maze)
    assert (mp[cells[:5, 0], cells[:5, 1]] == 1).all()
    assert (cells[:2, 0] * mp.shape[1] + cells[:2, 1] >= 128).all()
    q0 = sd['qpos'].cpu().numpy()
    assert (orc.xy_to_ij(q0[n - 1:])[0] < 0).any()  # off the map
    assert orc.physics(maze, q0, acts_np[0])[1][:5].all()  # inside a wall box: in contact
    acts = torch.tensor(acts_np, device=gpu)
    e_plain, e_gen = _loaded(gpu, n, maze, sd), _loaded(gpu, n, maze, sd)
    plain, plain_states = _plain_steps(e_plain, acts)
    gen, gen_states = _generic_steps(e_gen, acts)
    _assert_same(plain, plain_states, gen, gen_states)
    _assert_oracle(maze, sd, acts_np, plain, plain_states)
    e_plain.close()
    e_gen.close()


def test_no_table_survives_between_launches(gpu):
    """Handles of two mazes stepping alternately on one stream: each equals its solo run."""
    n, steps = 257, 4
    runs = {}
    for maze in ('medium', 'giant'):
        rng = np.random.RandomState(7 + len(maze))
        sd, acts_np, _ = _start(gpu, maze, n, False, rng)
        acts = torch.tensor(acts_np, device=gpu)
        solo = _loaded(gpu, n, maze, sd)
        want = []
        for t in range(steps):
            ob = solo.step(acts[t])[0]
            want.append((ob.cpu().numpy().copy(), _state(solo)))
        solo.close()
        runs[maze] = (_loaded(gpu, n, maze, sd), acts, want)
    got = {maze: [] for maze in runs}
    for t in range(steps):
        obs = {maze: runs[maze][0].step(runs[maze][1][t])[0] for maze in ('medium', 'giant')}  # back to back
        for maze in runs:
            got[maze].append((obs[maze].cpu().numpy().copy(), _state(runs[maze][0])))
    for maze, (env, _, want) in runs.items():
        for t in range(steps):
            assert np.array_equal(got[maze][t][0].view(np.uint8), want[t][0].view(np.uint8)), (maze, t)
            for key in STATE_KEYS:
                assert np.array_equal(got[maze][t][1][key], want[t][1][key]), (maze, t, key)
        env.close()
