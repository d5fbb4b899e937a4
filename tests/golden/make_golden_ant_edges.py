"""Generate tests/golden/antmaze_edges_golden.npz: the reference's antmaze
wrapper at its edges (tests/test_antmaze_cpu.py, tests/test_antmaze_edges_gpu.py).

Run in the build container (where the reference checkout exists), after the
oracle library is built (oracle/Makefile; the Philox draws come from it):
    python tests/golden/make_golden_ant_edges.py

The reference's own MazeEnv / AntEnv methods are executed through
make_golden_ant.py (ast-extracted, compiled with the reference's inheritance
over a stub MujocoEnv whose do_simulation loads a given post-physics state);
nothing of the reference is copied.  The recorder is extended here: it can
force a queue of `uniform` values (add_noise draws chosen by the generator or
taken from libogbx's Philox stream) and answers `randint` (the teleport's
out-portal index) from a queue.  Only inputs and outputs are saved, with the
provenance keys of make_golden_ant.py (src_sha256, ref_head).

Every block has n = 70 envs (one full 64-env kernel block plus a ragged one of
6) and is stored under `<block>_<timing>_<name>` for success_timing 'post' and
'pre'.  Inputs: seed, task, noise, body_draws, goal_states, qpos_post,
qvel_post (and task_xy, tp_draws, reset_states, reset_noise where used).
Outputs: reset_obs, reset_goal, reset_goal_ob, obs, reward, terminated,
truncated, success, body_qpos, body_qvel (the reference's data.qpos /
data.qvel after the step: body_qpos[..., :2] is get_xy()), and in the ep block
final_obs (elsewhere no env is reset and it would repeat obs).

  cfg1 / cfg2  large maze, T = 12, TimeLimit 8.  cfg1: terminate_at_goal=False;
        cfg2: reward_task_id=3, add_noise_to_goal=False, reset called with
        another task_id option (ignored).
  edge  large maze, 2 steps: step 0 feeds a designed xy, step 1 a far one, so
        'post' shows the verdict at step 0 and 'pre' at step 1.  `edge_class`:
        0 plain, 1 (a) rows on which sqrt(fma(dy,dy,dx*dx)) <= 0.5 and
        sqrt(dx*dx+dy*dy) <= 0.5 disagree, 2 (b) an integer goal centre with xy
        at distance exactly 0.5 and one ulp either side, 3 (c) NaN / inf xy.
  tp    teleport maze, T = 16: paths enter both in-portals, rows on the 1.5
        circle where the two roundings disagree (`tp_circle` rows), out-portal
        indices as libogbx draws them, half the envs with a task_info whose
        goal cell is an out-portal cell.
  ep    large maze, T = 28, TimeLimit 7: the reference's host loop, step and
        reset(options={'task_id': same}) when terminated or truncated, the
        reset's add_noise draws being libogbx's auto-reset draws.

Non-xy body coordinates are only ever copied by the wrapper: they are multiples
of 1/64, different per (step, env, column), and every recorded draw is
quantised to a short binary fraction, so that the file compresses.
"""

import io
import json
import os
import sys
import zipfile
from fractions import Fraction

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
for p in (OUT, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_ant as base  # noqa: E402
from make_golden_ant import _NP, _Rec, build_classes, make_env  # noqa: E402
from oracle import locomaze as orc  # noqa: E402

N = 70
TAG_TELEPORT = 0x4D5A0002
MAX_BYTES = 1_000_000


class _QRec(_Rec):
    """_Rec that answers scalar `uniform` calls from a forced queue while one
    is set, and `randint` from a queue of out-portal indices."""

    def __init__(self, rng):
        super().__init__(rng)
        self.forced = []
        self.ints = []

    def uniform(self, low=0.0, high=1.0, size=None):
        if self.forced:
            assert size is None
            v = float(self.forced.pop(0))
            assert low <= v <= high
            self.log.append(('uniform', np.array(v, np.float64)))
            return v
        return super().uniform(low, high, size)

    def randint(self, *a, **k):
        v = int(self.ints.pop(0))
        self.log.append(('randint', v))
        return v


class _ShortRng:
    """The env's np_random: draws quantised to short binary fractions (1/1024
    for uniforms, 1/8 for normals), so the recorded states compress."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)

    def uniform(self, low, high, size=None):
        return np.clip(np.round(self.rng.uniform(low, high, size) * 1024) / 1024, low, high)

    def standard_normal(self, size=None):
        return np.round(self.rng.standard_normal(size) * 8) / 8


def filler(t, i, cols, salt):
    """Body coordinates that the wrapper only copies: multiples of 1/64,
    different per (step, env, column)."""
    return (salt * 4096 + (t * N + i) * 32 + np.arange(cols)) / 64.0


def body_row(t, i, xy, salt=0):
    q = filler(t, i, 15, salt)
    q[:2] = xy
    return q, filler(t, i, 29, salt)[15:] + 0.25


def grid(xy):
    return np.round(np.asarray(xy, np.float64) * 1024) / 1024


def verdicts(dx, dy, tol):
    """(sqrt(fma(dy,dy,dx*dx)) <= tol, sqrt(dx*dx+dy*dy) <= tol,
    sqrt(fma(dx,dx,dy*dy)) <= tol) with every sum rounded once, exactly."""
    dx, dy = float(dx), float(dy)
    a = float(Fraction(dy) ** 2 + Fraction(dx * dx))
    b = dx * dx + dy * dy
    c = float(Fraction(dx) ** 2 + Fraction(dy * dy))
    return tuple(bool(np.sqrt(s) <= tol) for s in (a, b, c))


def circle_row(rng, centre, tol, outcome):
    """An xy on the circle of radius tol about `centre`, x nudged by up to 6
    ulps, on which the fma(dy,dy,dx*dx) rounding gives `outcome` and the plain
    rounding the opposite.  Returns (xy [2], trials)."""
    trials = 0
    while True:
        trials += 1
        assert trials < 200000
        th = rng.uniform(0, 2 * np.pi)
        x = centre[0] + tol * np.cos(th)
        y = centre[1] + tol * np.sin(th)
        for _ in range(int(rng.randint(0, 7))):
            x = np.nextafter(x, np.inf if rng.rand() < 0.5 else -np.inf)
        fa, pl, _ = verdicts(x - centre[0], y - centre[1], tol)
        if fa != pl and fa == outcome:
            return np.array([x, y]), trials


class Block:
    """Arrays of one (block, timing) and the reference loop that fills them."""

    def __init__(self, T, seed, with_resets=False):
        self.T, self.seed, self.with_resets = T, seed, with_resets
        z = np.zeros
        self.a = dict(seed=np.array(seed, np.int64), task=z(N, np.int32), noise=z((N, 4)), body_draws=z((N, 29)),
                      goal_states=z((N, 29)), reset_obs=z((N, 29)), reset_goal=z((N, 2)), reset_goal_ob=z((N, 29)),
                      qpos_post=z((T, N, 15)), qvel_post=z((T, N, 14)), obs=z((T, N, 29)),
                      reward=z((T, N), np.float32), terminated=z((T, N), np.uint8), truncated=z((T, N), np.uint8),
                      success=z((T, N), np.uint8), body_qpos=z((T, N, 15)), body_qvel=z((T, N, 14)))
        if with_resets:  # only the host loop has a final observation that differs from obs
            self.a['final_obs'] = z((T, N, 29))
            self.a['reset_states'] = np.full((T, N, 29), np.nan)
            self.a['reset_noise'] = np.full((T, N, 4), np.nan)

    def reset(self, env, rec, i, options, noise, salt):
        """env.reset with the add_noise draws forced to `noise` and the five
        goal-phase states fed.  Returns (ob, info, the second reset_model's
        draws [29], the goal-phase state [29])."""
        five = [body_row(-1 - k, i, (0.0, 0.0), salt) for k in range(5)]
        env._feed = iter(five)
        rec.forced = [float(x) for x in noise]
        rec.log.clear()
        env.np_random.log.clear()
        ob, info = env.reset(options=options)
        assert not rec.forced
        draws = env.np_random.log[-2:]  # the second reset_model: uniform(15), normal(14)
        assert draws[0][0] == 'uniform' and draws[1][0] == 'normal'
        bd = np.concatenate([draws[0][1], draws[1][1]])
        return ob, info, bd, np.concatenate(five[-1])

    def first_reset(self, env, rec, i, options, noise, noise_stored=None):
        a = self.a
        ob, info, bd, gs = self.reset(env, rec, i, options, noise, salt=1)
        a['noise'][i] = noise if noise_stored is None else noise_stored
        a['body_draws'][i], a['goal_states'][i] = bd, gs
        a['reset_obs'][i], a['reset_goal'][i], a['reset_goal_ob'][i] = ob, env.cur_goal_xy, info['goal']

    def step(self, env, t, i, q, v):
        a = self.a
        a['qpos_post'][t, i], a['qvel_post'][t, i] = q, v
        env._feed = iter([(q, v)])
        o, r, te, tr, info = env.step(np.zeros(8))
        a['obs'][t, i] = o
        if self.with_resets:
            a['final_obs'][t, i] = o
        a['reward'][t, i], a['terminated'][t, i], a['success'][t, i] = r, te, info['success']
        a['body_qpos'][t, i], a['body_qvel'][t, i] = env.data.qpos, env.data.qvel
        assert np.array_equal(env.get_xy(), env.data.qpos[:2], equal_nan=True)
        return te

    def after_reset(self, env, t, i, ob, bd, noise):
        a = self.a
        a['obs'][t, i] = ob
        a['body_qpos'][t, i], a['body_qvel'][t, i] = env.data.qpos, env.data.qvel
        st = np.concatenate([env.init_qpos + bd[:15], env.init_qvel + 0.1 * bd[15:]])  # reset_model, before set_xy
        assert np.array_equal(st[2:], ob[2:])
        a['reset_states'][t, i] = st
        a['reset_noise'][t, i] = noise


def new_env(cls, rec, maze, timing, seed, **attrs):
    env = make_env(cls, maze, iter(()), _Rec(_ShortRng(seed)), timing)
    for k, v in attrs.items():
        setattr(env, '_' + k, v)
    return env


def block_cfg(rng, timing, cfg, max_steps=8, T=12):
    rec = _QRec(None)
    cls = build_classes(_NP(rec))
    b = Block(T, seed=int(rng.randint(1 << 30)))
    for i in range(N):
        attrs = (dict(terminate_at_goal=False, add_noise_to_goal=True) if cfg == 1 else
                 dict(terminate_at_goal=True, add_noise_to_goal=False, reward_task_id=3))
        env = new_env(cls, rec, 'large', timing, int(rng.randint(1 << 30)), **attrs)
        task = i % 5 + 1  # cfg2: the option differs from reward_task_id for 4 envs in 5 and is ignored
        noise = rng.uniform(-1, 1, 4)
        b.a['task'][i] = task
        b.first_reset(env, rec, i, dict(task_id=task), noise[:4 if cfg == 1 else 2], noise_stored=noise)
        if cfg == 2:
            assert env.cur_task_id == 3
        xy0, goal = np.array(env.get_xy()), np.array(env.cur_goal_xy)
        elapsed = 0
        for t in range(T):
            if i % 2 == 0:  # walks onto the goal
                xy = grid(xy0 + (goal - xy0) * min(1.0, (t + 1) / (3 + i % 7)) + rng.uniform(-0.2, 0.2, 2))
            else:
                xy = grid(xy0 + rng.uniform(-2, 2, 2))
            b.step(env, t, i, *body_row(t, i, xy))
            elapsed += 1  # gymnasium TimeLimit
            b.a['truncated'][t, i] = elapsed >= max_steps
    a = b.a
    assert a['success'].sum() >= 40 and a['truncated'].sum() >= 70, (a['success'].sum(), a['truncated'].sum())
    if cfg == 1:
        assert a['terminated'].sum() == 0
    else:
        assert set(np.unique(a['reward'])) == {-1.0, 0.0}
        assert np.array_equal(a['terminated'], a['success'])
    a['max_steps'] = np.array(max_steps, np.int32)
    return a


EDGE_PLAIN, EDGE_A, EDGE_B, EDGE_C = 0, 1, 2, 3


def block_edge(rng, timing, design):
    rec = _QRec(None)
    cls = build_classes(_NP(rec))
    b = Block(2, seed=int(rng.randint(1 << 30)))
    kinds, noises, xys = design
    for i in range(N):
        env = new_env(cls, rec, 'large', timing, int(rng.randint(1 << 30)))
        task = i % 5 + 1
        b.a['task'][i] = task
        b.first_reset(env, rec, i, dict(task_id=task), noises[i])
        b.step(env, 0, i, *body_row(0, i, xys[i]))
        b.step(env, 1, i, *body_row(1, i, grid(np.array(env.cur_goal_xy) + (3.0, -2.5))))
    a = b.a
    a['max_steps'] = np.array(1000, np.int32)
    verdict = a['success'][0 if timing == 'post' else 1]
    assert not a['success'][1 if timing == 'post' else 0].any()
    goal = a['reset_goal']
    ka = np.nonzero(kinds == EDGE_A)[0]
    agree = np.zeros(3, int)
    for i in ka:
        v = verdicts(xys[i, 0] - goal[i, 0], xys[i, 1] - goal[i, 1], 0.5)
        assert v[0] != v[1]
        agree += [bool(verdict[i]) == x for x in v]
    # the reference (np.linalg.norm) rounds as sqrt(fma(dy, dy, dx*dx)) on every class (a) row
    assert agree[0] == len(ka), agree
    assert len(ka) >= 16 and verdict[ka].sum() >= 4 and (1 - verdict[ka]).sum() >= 4
    assert not verdict[kinds == EDGE_C].any() and (kinds == EDGE_C).sum() >= 8
    return a, agree


def design_edge(rng):
    """Per env: class, forced add_noise draws and the designed xy of step 0."""
    from oracle import antmaze_np as am

    kinds = np.array([EDGE_A] * 32 + [EDGE_B] * 12 + [EDGE_C] * 10 + [EDGE_PLAIN] * 16)
    kinds = kinds[rng.permutation(N)]
    noises = rng.uniform(-1, 1, (N, 4))
    noises[kinds == EDGE_B, 2:] = 0.0  # the goal is the integer cell centre
    xys = np.zeros((N, 2))
    tasks = am.LARGE_TASKS[np.arange(N) % 5]
    goal = np.stack(am.ij_to_xy(tasks[:, 2], tasks[:, 3]), 1) + noises[:, 2:] * 4.0 / 4
    trials, na, nb, nc, npl = 0, 0, 0, 0, 0
    bad = [(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, 1.0), (-np.inf, 1.0), (1.0, np.inf),
           (1.0, -np.inf), (np.inf, -np.inf), (-np.inf, np.nan), (np.inf, np.inf)]
    for i in range(N):
        g = goal[i]
        if kinds[i] == EDGE_A:
            xys[i], k = circle_row(rng, g, 0.5, na % 2 == 0)  # alternate the outcomes
            na += 1
            trials += k
        elif kinds[i] == EDGE_B:
            axis, sign, nudge = nb % 2, 1 - 2 * (nb // 2 % 2), nb // 4  # 0 exact, 1 outward, 2 inward
            xy = g.copy()
            xy[axis] = g[axis] + sign * 0.5
            if nudge:
                xy[axis] = np.nextafter(xy[axis], xy[axis] + sign * (1 if nudge == 1 else -1))
            xys[i] = xy
            nb += 1
        elif kinds[i] == EDGE_C:
            xys[i] = bad[nc]
            nc += 1
        else:
            xys[i] = g if npl % 2 == 0 else g + (0.5 + (1e-9 if npl % 4 == 1 else -1e-9), 0.0)
            npl += 1
    return (kinds, noises, xys), trials


def tp_index(seed, i, episode, elapsed, n_out):
    """The out-portal index libogbx draws for global env i at that step."""
    k0, k1 = orc.philox_key(seed, orc.TAG_MAZE_RESET)
    w = orc.philox4x32([i & 0xFFFFFFFF, episode, 0x100 + elapsed, i >> 32], k0 ^ TAG_TELEPORT, k1)
    return (int(w[0]) * n_out) >> 32


def block_tp(rng, timing, circle, T=16):
    from oracle import antmaze_np as am

    info = json.load(open(os.path.join(OUT, 'teleport_golden.json')))
    ins, outs, radius = am.teleport_table(info)
    info = dict(info, teleport_in_xys=[tuple(x) for x in ins], teleport_out_xys=[tuple(x) for x in outs])
    rec = _QRec(None)
    cls = build_classes(_NP(rec))
    seed = int(rng.randint(1 << 30))
    b = Block(T, seed=seed)
    a = b.a
    a['task_xy'] = np.zeros((N, 4))
    a['tp_draws'] = np.zeros((T, N), np.int32)
    a['tp_circle'] = np.zeros((T, N), np.uint8)
    tele = np.zeros((T, N), np.int8) - 1
    for i in range(N):
        env = new_env(cls, rec, 'teleport', timing, int(rng.randint(1 << 30)), teleport_info=info)
        a['tp_draws'][:, i] = [tp_index(seed, i, 1, t, len(outs)) for t in range(T)]
        plan = {t: (i + t // 4) % 2 for t in range(T) if (t + i) % 4 == 0}  # step -> in-portal entered
        first = min(plan)
        noise = rng.uniform(-1, 1, 4)
        if i % 2 == 1:
            # a task_info whose goal cell is the out-portal cell of the first teleport, goal noise small:
            # under 'pre' the step after succeeds only if the stored xy is that out-portal
            o = a['tp_draws'][first, i]
            ti = dict(init_ij=(1 + i % 3, 1 + i % 5), goal_ij=tuple(info['teleport_out_ijs'][o]))
            noise[2:] = rng.uniform(-0.3, 0.3, 2)
            options = dict(task_info=ti)
            a['task_xy'][i] = [*env.ij_to_xy(ti['init_ij']), *env.ij_to_xy(ti['goal_ij'])]
        else:
            task = i % 5 + 1
            a['task'][i] = task
            options = dict(task_id=task)
            tinfo = env.task_infos[task - 1]
            a['task_xy'][i] = [*tinfo['init_xy'], *tinfo['goal_xy']]
        b.first_reset(env, rec, i, options, noise)
        for t in range(T):
            if (t, i) in circle:
                xy = circle[(t, i)]
                a['tp_circle'][t, i] = 1
            elif t in plan:
                xy = grid(ins[plan[t]] + rng.uniform(-1.0, 1.0, 2))
            else:
                xy = grid((8.0 + i % 3, 4.0) + rng.uniform(-2, 2, 2))  # far from both in-portals
            rec.ints = [a['tp_draws'][t, i]]
            b.step(env, t, i, *body_row(t, i, xy))
            moved = not np.array_equal(a['body_qpos'][t, i, :2], xy)
            assert moved == (not rec.ints)
            if moved:
                p = int(np.argmin(np.abs(ins - xy).sum(1)))
                tele[t, i] = p
                assert np.array_equal(a['body_qpos'][t, i, :2], outs[a['tp_draws'][t, i]])
    a['max_steps'] = np.array(1000, np.int32)
    used = a['tp_draws'][tele >= 0]
    assert all((used == o).sum() >= 5 for o in range(len(outs))), np.bincount(used)
    assert all(((tele == p).any(0)).sum() >= 10 for p in range(len(ins)))
    cv = [(bool(tele[t, i] >= 0)) for (t, i) in circle]
    assert len(cv) >= 8 and 0 < sum(cv) < len(cv)
    for (t, i), xy in circle.items():  # the reference rounds the portal distance as the documented form does
        p = int(np.argmin(np.abs(ins - xy).sum(1)))
        v = verdicts(xy[0] - ins[p, 0], xy[1] - ins[p, 1], 1.5 * radius)
        assert v[0] != v[1] and v[0] == (tele[t, i] >= 0)
    if timing == 'pre':
        firsts = [(min(t for t in range(T) if (t + i) % 4 == 0), i) for i in range(1, N, 2)]
        wins = sum(int(a['success'][t + 1, i]) for t, i in firsts if tele[t, i] >= 0 and t + 1 < T)
        assert wins >= 10, wins
    return a


def design_tp_circle(rng):
    """(step, env) -> xy on the 1.5 circle of an in-portal where the two
    roundings disagree; placed on steps the paths leave free."""
    from oracle import antmaze_np as am

    ins, _, radius = am.teleport_table(json.load(open(os.path.join(OUT, 'teleport_golden.json'))))
    out = {}
    for k in range(12):
        i = 3 + 5 * k  # envs of both kernel blocks (3 .. 58) and, below, the ragged one
        i = i if k < 11 else 67
        t = next(t for t in range(2, 16) if (t + i) % 4 == 2)
        out[(t + 4 * (k % 3), i)] = circle_row(rng, ins[k % 2], 1.5 * radius, k // 2 % 2 == 0)[0]
    return out


def block_ep(rng, timing, T=28, max_steps=7):
    rec = _QRec(None)
    cls = build_classes(_NP(rec))
    seed = int(rng.randint(1 << 30))
    b = Block(T, seed=seed, with_resets=True)
    a = b.a
    episodes = np.zeros(N, int)
    for i in range(N):
        env = new_env(cls, rec, 'large', timing, int(rng.randint(1 << 30)))
        task = i % 5 + 1
        a['task'][i] = task
        e = 1
        b.first_reset(env, rec, i, dict(task_id=task), orc.reset_draws(1, seed, env_base=i, episode=e)[0])
        elapsed = 0
        for t in range(T):
            # the env stands on its goal on step `hit` of its episode (7: terminated and truncated at
            # once; 8, 9: never, truncated only); under 'pre' one step earlier, the verdict coming a step late
            hit = (i * 5 + e * 3) % 9 + 1
            goal = np.array(env.cur_goal_xy)
            on = elapsed + 1 == (hit if timing == 'post' else hit - 1)
            xy = grid(goal + rng.uniform(-0.25, 0.25, 2)) if on else grid(goal + (2.0, 1.5) + rng.uniform(-1, 1, 2))
            te = b.step(env, t, i, *body_row(t, i, xy))
            elapsed += 1
            tr = elapsed >= max_steps
            a['truncated'][t, i] = tr
            if te or tr:
                e += 1
                episodes[i] += 1
                noise = orc.reset_draws(1, seed, env_base=i, episode=e)[0]
                ob, _, bd, _ = b.reset(env, rec, i, dict(task_id=task), noise, salt=2 + t)
                b.after_reset(env, t, i, ob, bd, noise)
                elapsed = 0
    ends = (a['terminated'] | a['truncated']).astype(bool)
    both = (a['terminated'] & a['truncated']).astype(bool)
    assert episodes.min() >= 3 and a['terminated'].sum() >= 60 and a['truncated'].sum() >= 100, (
        episodes.min(), a['terminated'].sum(), a['truncated'].sum())
    assert both.sum() >= 4 and ends[:, 64:].any(), both.sum()
    assert np.array_equal(~np.isnan(a['reset_states'][:, :, 0]), ends)
    a['max_steps'] = np.array(max_steps, np.int32)
    return a


def build():
    rng = np.random.RandomState(20261020)
    out = {}
    edge_design, trials = design_edge(rng)
    circle = design_tp_circle(rng)
    agree = None
    for timing in ('post', 'pre'):
        blocks = {'cfg1': block_cfg(rng, timing, 1), 'cfg2': block_cfg(rng, timing, 2)}
        blocks['edge'], agree = block_edge(rng, timing, edge_design)
        blocks['tp'] = block_tp(rng, timing, circle)
        blocks['ep'] = block_ep(rng, timing)
        for name, arrs in blocks.items():
            out.update({f'{name}_{timing}_{k}': v for k, v in arrs.items()})
    out['edge_class'] = edge_design[0].astype(np.uint8)
    out['src_sha256'] = np.array(sorted(f'{k} {v}' for k, v in base._PROVENANCE.items()))
    out['ref_head'] = np.array(base._ref_head())
    return out, trials, agree


def save_npz(path, arrays):
    """np.savez_compressed with LZMA members (np.load reads them as it reads
    deflated ones) and fixed timestamps: deflate leaves this file near 1.8 MB,
    every 8-byte value differing from its neighbours in a byte or two."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_LZMA) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        compress_type=zipfile.ZIP_LZMA)


def main():
    out, trials, agree = build()
    path = os.path.join(OUT, 'antmaze_edges_golden.npz')
    save_npz(path, out)
    size = os.path.getsize(path)
    print(f'{path}: {size} bytes, {len(out)} arrays')
    print(f'class (a): {int((out["edge_class"] == EDGE_A).sum())} rows in {trials} trials; the reference agrees with '
          f'fma(dy,dy,dx*dx) / plain / fma(dx,dx,dy*dy) on {agree[0]} / {agree[1]} / {agree[2]}')
    for b in ('cfg1', 'cfg2', 'edge', 'tp', 'ep'):
        for t in ('post', 'pre'):
            print(b, t, *(f'{k} {int(out[f"{b}_{t}_{k}"].sum())}' for k in ('success', 'terminated', 'truncated')))
    assert size <= MAX_BYTES, size


if __name__ == '__main__':
    main()
