"""GPU parity at the antmaze wrapper's edges (csrc/antmaze.h: ant_reset_kernel,
ant_step_kernel<kVec>) against tests/golden/antmaze_edges_golden.npz, the
reference's own MazeEnv / AntEnv methods run by make_golden_ant_edges.py.

Blocks of 70 envs (one full 64-env kernel block and a ragged one of 6), each
for success_timing 'post' and 'pre':
  cfg1 / cfg2  terminate_at_goal=False; single-task reward with the task_id
               option ignored and add_noise_to_goal=False
  edge         xy within an ulp of the success circle (the fma rounding against
               the plain one, distance exactly 0.5 and an ulp either side),
               NaN / inf xy
  tp           the teleport maze: both in-portals, rows on the 1.5 circle, the
               Philox out-portal, task_info goals on out-portal cells
  ep           the reference's step / reset host loop against same-step
               auto-reset, envs that terminate and truncate at once included
and each in three buffer modes: fresh 16-byte-aligned inputs (the kVec path),
inputs offset by one double (the scalar path) -- both through the C-ABI with
outputs allocated here between sentinel margins -- and in place through
body_state() and wrap_step.  Everything is compared bit for bit.

Then what the reference cannot give: a masked reset, a replay of the Philox
body draws from their counter words, and device-drawn tasks.
"""

import numpy as np
import pytest
import torch

import antmaze_edges_util as eu
import ogbench_amd
from ogbench_amd import _lib

pytestmark = pytest.mark.gpu

MARGIN = 64  # elements either side of every buffer allocated here
SENTINEL = {torch.float64: -7.25e77, torch.float32: -3.5e33, torch.uint8: 0xA5}


class Guarded:
    """A device buffer between two sentinel margins; `offset` elements shift
    the view (one double: off 16-byte alignment)."""

    def __init__(self, shape, dtype, device, offset=0):
        self.numel = int(np.prod(shape))
        self.lo = MARGIN + offset
        self.sent = SENTINEL[dtype]
        self.buf = torch.full((self.lo + self.numel + MARGIN,), self.sent, dtype=dtype, device=device)
        self.view = self.buf[self.lo:self.lo + self.numel].view(*shape)
        assert (self.view.data_ptr() % 16 == 0) == (offset == 0)

    def fill(self):
        self.view.fill_(self.sent)

    def margins_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == self.sent).all() and (b[self.lo + self.numel:] == self.sent).all())


def _np(t):
    return t.cpu().numpy()


def _make_env(gpu, name, timing, g, **kw):
    return ogbench_amd.MazeEnv('ant', eu.MAZE[name], num_envs=eu.N, device=gpu, success_timing=timing,
                               max_episode_steps=int(g['max_steps']), auto_reset=name == 'ep', **eu.CONFIG[name], **kw)


def _reset_options(name, g):
    opts = dict(body_draws=torch.tensor(g['body_draws']), goal_states=torch.tensor(g['goal_states']))
    if name == 'tp':  # task_info rows: the table's cell centres, or an out-portal cell as the goal
        opts.update(task_info=torch.tensor(g['task_xy']), noise=torch.tensor(g['noise']))
    elif name == 'ep':  # the add_noise draws are the handle's own Philox draws for the stored seed
        opts.update(task_id=torch.tensor(g['task']))
    else:  # cfg2: the task_id option differs from reward_task_id and is ignored
        opts.update(task_id=torch.tensor(g['task']), noise=torch.tensor(g['noise']))
    return opts


@pytest.mark.parametrize('mode', ['vec', 'scalar', 'inplace'])
@pytest.mark.parametrize('timing', eu.TIMINGS)
@pytest.mark.parametrize('name', eu.BLOCKS)
def test_block_matches_reference(gpu, name, timing, mode):
    g = eu.block(name, timing)
    n, T = eu.N, g['obs'].shape[0]
    env = _make_env(gpu, name, timing, g)
    orb = eu.oracle_batch(name, timing, g)  # only for cur_goal_xy after the loop's resets
    obs, info = env.reset(seed=int(g['seed']), options=_reset_options(name, g))
    assert eu.same_bits(_np(obs), g['reset_obs'])
    assert eu.same_bits(_np(info['goal']), g['reset_goal_ob'])
    assert eu.same_bits(_np(env.cur_goal_xy), g['reset_goal'])
    assert eu.same_bits(_np(env.get_xy()), g['reset_obs'][:, :2])
    bq, bv = env.body_state()
    assert eu.same_bits(_np(bq), g['reset_obs'][:, :15]) and eu.same_bits(_np(bv), g['reset_obs'][:, 15:])
    auto = int(name == 'ep')
    f64, f32, u8 = torch.float64, torch.float32, torch.uint8
    if mode != 'inplace':
        off = int(mode == 'scalar')
        qin, vin = Guarded((n, 15), f64, gpu, off), Guarded((n, 14), f64, gpu, off)
        rsin = Guarded((n, 29), f64, gpu)
        out = dict(obs=Guarded((n, 29), f64, gpu), reward=Guarded((n,), f32, gpu), term=Guarded((n,), u8, gpu),
                   trunc=Guarded((n,), u8, gpu), succ=Guarded((n,), u8, gpu), final=Guarded((n, 29), f64, gpu))
        guards = [qin, vin, rsin, *out.values()]
    for t in range(T):
        q, v = torch.tensor(g['qpos_post'][t], device=gpu), torch.tensor(g['qvel_post'][t], device=gpu)
        rs = torch.tensor(g['reset_states'][t], device=gpu) if auto else None  # NaN rows for envs that go on
        if mode == 'inplace':  # the physics engine overwrote the handle's state
            bq.copy_(q)
            bv.copy_(v)
            o, r, te, tr, inf = env.wrap_step(bq, bv, reset_states=rs)
            su, fin = inf['success'], inf.get('final_observation')
        else:
            qin.view.copy_(q)
            vin.view.copy_(v)
            for x in out.values():
                x.fill()
            if auto:
                rsin.view.copy_(rs)
            _lib.check(env._L.ogbx_antmaze_step(
                env._h, qin.view.data_ptr(), vin.view.data_ptr(), out['obs'].view.data_ptr(),
                out['reward'].view.data_ptr(), out['term'].view.data_ptr(), out['trunc'].view.data_ptr(),
                out['succ'].view.data_ptr(), out['final'].view.data_ptr(), auto,
                rsin.view.data_ptr() if auto else None, env._stream()), 'ogbx_antmaze_step')
            o, r, te, tr, su, fin = (out[k].view for k in ('obs', 'reward', 'term', 'trunc', 'succ', 'final'))
        eu.oracle_step(name, orb, g, t)
        o, fin = _np(o), None if fin is None else _np(fin)
        assert eu.same_bits(o, g['obs'][t]), t
        assert eu.same_bits(_np(r), g['reward'][t]), t
        assert np.array_equal(_np(te).astype(np.uint8), g['terminated'][t]), t
        assert np.array_equal(_np(tr).astype(np.uint8), g['truncated'][t]), t
        assert np.array_equal(_np(su).astype(np.uint8), g['success'][t]), t
        # the body state after the step: a teleport's set_xy, an auto-reset's whole rows
        assert eu.same_bits(_np(bq), g['body_qpos'][t]), t
        assert eu.same_bits(_np(bv), g['body_qvel'][t]), t
        assert eu.same_bits(_np(env.get_xy()), g['body_qpos'][t][:, :2]), t
        assert eu.same_bits(_np(env.cur_goal_xy), orb.goal), t
        if auto:
            ends = (g['terminated'][t] | g['truncated'][t]).astype(bool)
            assert eu.same_bits(fin[ends], g['final_obs'][t][ends]), t
            if mode != 'inplace':  # rows of envs that go on are not written
                assert (fin[~ends] == out['final'].sent).all(), t
            # the NaN filler of the unused reset_states rows appears nowhere
            assert not any(np.isnan(x).any() for x in (o, fin[ends], _np(bq), _np(bv))), t
        if mode != 'inplace':  # the inputs are read only
            assert eu.same_bits(_np(qin.view), g['qpos_post'][t]) and eu.same_bits(_np(vin.view), g['qvel_post'][t])
    if mode != 'inplace':
        assert all(x.margins_intact() for x in guards)


def test_edge_rows_cover_their_classes(gpu):
    """What the edge block pins, spelled out on the device's verdicts: the
    class (a) rows are exactly those a plain dx*dx + dy*dy would get wrong, the
    class (b) rows at distance exactly 0.5 succeed (<=), NaN / inf rows fail."""
    kinds = eu.load()['edge_class']
    g = eu.block('edge', 'post')
    env = _make_env(gpu, 'edge', 'post', g)
    env.reset(seed=0, options=_reset_options('edge', g))
    q, v = torch.tensor(g['qpos_post'][0], device=gpu), torch.tensor(g['qvel_post'][0], device=gpu)
    succ = _np(env.wrap_step(q, v)[4]['success'])
    xy, goal = g['qpos_post'][0][:, :2], g['reset_goal']
    dx, dy = xy[:, 0] - goal[:, 0], xy[:, 1] - goal[:, 1]
    a, b, c = kinds == eu.EDGE_A, kinds == eu.EDGE_B, kinds == eu.EDGE_C
    assert np.array_equal(succ[a], ~(np.sqrt(dx[a] * dx[a] + dy[a] * dy[a]) <= 0.5))
    r = np.maximum(np.abs(dx[b]), np.abs(dy[b]))
    assert succ[b][r == 0.5].all() and (r == 0.5).sum() == 4 and not succ[b][r > 0.5].any()
    assert not succ[c].any()


def _state(env):
    sd = env.state_dict()
    return {k: _np(v) for k, v in sd.items() if k != 'seed'}


def test_masked_reset(gpu):
    """reset(mask=): unmasked envs keep body state, goal, elapsed, task,
    episode counter and goal observation; masked ones equal a full reset of a
    twin handle; with seed= only the masked Philox counters restart."""
    n, seed = 130, 11
    rng = np.random.RandomState(5)
    tid1 = torch.tensor((np.arange(n) % 5 + 1).astype(np.int32))
    tid2 = torch.tensor(((np.arange(n) + 2) % 5 + 1).astype(np.int32))
    mask = rng.rand(n) < 0.5
    mask2 = rng.rand(n) < 0.5
    assert 40 < mask.sum() < 90 and mask[64:128].any() and not mask[64:128].all() and mask[128:].any()
    a, b, c = (ogbench_amd.MazeEnv('ant', 'large', num_envs=n, device=gpu) for _ in range(3))
    for e in (a, b):
        e.reset(seed=seed, options=dict(task_id=tid1))
    for _ in range(2):  # elapsed = 2, the body state = what the engine left
        q = torch.tensor(rng.normal(size=(n, 15)) + 50.0, device=gpu)
        v = torch.tensor(rng.normal(size=(n, 14)), device=gpu)
        a.wrap_step(q, v)
    before, goal_ob0 = _state(a), _np(a._goal_ob).copy()
    obs, info = a.reset(options=dict(task_id=tid2), mask=torch.tensor(mask))
    obs, goal_ob, after = _np(obs).copy(), _np(info['goal']).copy(), _state(a)
    fobs, finfo = b.reset(options=dict(task_id=tid2))  # the twin: a full second reset
    fobs, fgoal_ob, full = _np(fobs), _np(finfo['goal']), _state(b)
    assert (before['elapsed'] == 2).all() and (before['episode'] == 1).all()
    for k in before:
        assert eu.same_bits(after[k][~mask], before[k][~mask]), k
        assert eu.same_bits(after[k][mask], full[k][mask]), k
    assert eu.same_bits(goal_ob[~mask], goal_ob0[~mask]) and eu.same_bits(goal_ob[mask], fgoal_ob[mask])
    assert eu.same_bits(obs[mask], fobs[mask])
    assert (after['episode'] == 1 + mask).all() and (after['elapsed'][mask] == 0).all()
    assert np.array_equal(after['task'], np.where(mask, _np(tid2), _np(tid1)))
    # seed=: the masked counters restart, the others go on
    obs, info = a.reset(seed=99, options=dict(task_id=tid1), mask=torch.tensor(mask2))
    obs, goal_ob, last = _np(obs).copy(), _np(info['goal']).copy(), _state(a)
    cobs, cinfo = c.reset(seed=99, options=dict(task_id=tid1))
    fresh = _state(c)
    assert np.array_equal(last['episode'], np.where(mask2, 1, after['episode']))
    for k in after:
        assert eu.same_bits(last[k][~mask2], after[k][~mask2]), k
        assert eu.same_bits(last[k][mask2], fresh[k][mask2]), k
    assert eu.same_bits(obs[mask2], _np(cobs)[mask2]) and eu.same_bits(goal_ob[mask2], _np(cinfo['goal'])[mask2])


# Largest distance seen on an MI355X between a velocity draw and the long-double
# Box-Muller of the same uniforms, in ulps (test_body_draws_replay prints it):
# 2.623 over the 64-env case, 1.691 over the 8-env one.
MEASURED_ULP = 2.623
ULP_BOUND = min(4 * MEASURED_ULP, 16.0)


@pytest.mark.parametrize('n,env_base', [(64, 0), (8, 2**32 + 5)])
def test_body_draws_replay(gpu, n, env_base):
    """The Philox body draws replayed from their counter words: counter (gi lo,
    episode, slot + c, gi hi), key (k0 ^ 0x414E0001, k1), u01_from on the word
    pairs (x, y) and (z, w); slot 0x300 for the returned ob and 0x340 for the
    goal observation, for two episodes.  The 13 free uniform coordinates
    (qpos0 + (-0.1 + 0.2 u0)) are exact double arithmetic and compared bit for
    bit; the 14 normals are held to a np.longdouble Box-Muller of the same
    uniforms within ULP_BOUND = 4 x the largest distance measured on the device
    (MEASURED_ULP above: 2.623 ulp on an MI355X, the device's log1p, sqrt,
    cospi and the two roundings of r * c and 0.1 * z together, so the bound is
    10.5 ulp; at most 16 ulp).  A wrong slot, word pair or a lost
    high word of the global env index is an O(1) error."""
    seed = 2026
    env = ogbench_amd.MazeEnv('ant', 'large', num_envs=n, device=gpu, env_base=env_base)
    worst = 0.0
    for episode in (1, 2):
        obs, info = env.reset(seed=seed if episode == 1 else None, options=dict(task_id=2))
        obs, gob = _np(obs), _np(info['goal'])
        assert eu.same_bits(gob[:, :2], _np(env.cur_goal_xy)) and eu.same_bits(obs[:, :2], _np(env.get_xy()))
        for i in range(n):
            for got, slot in ((obs[i], 0x300), (gob[i], 0x340)):
                q, vel = eu.body_state_from_uniforms(eu.body_uniforms(seed, env_base + i, episode, slot))
                assert eu.same_bits(got[2:15], q[2:]), (i, slot)
                d = eu.ulp_distance(got[15:], vel).max()
                worst = max(worst, float(d))
                assert d <= ULP_BOUND, (i, slot, d)
        assert not np.any(gob[:, 2:] == obs[:, 2:])  # the goal observation has its own draws
    print(f'largest ulp distance of a velocity draw: {worst:.3f}')


def test_device_drawn_tasks_match_point_handle(gpu):
    """Without a task_id the ant handle draws the tasks (and the init / goal
    xy) the point handle draws for the same seed and env_base: draw_task and
    reset_draws are shared."""
    n, seed, base = 130, 31, 7
    ant = ogbench_amd.MazeEnv('ant', 'large', num_envs=n, device=gpu, env_base=base)
    point = ogbench_amd.MazeEnv('point', 'large', num_envs=n, device=gpu, env_base=base)
    for episode in (1, 2):
        ant.reset(seed=seed if episode == 1 else None)
        point.reset(seed=seed if episode == 1 else None)
        sa, sp = ant._state_views(), point._state_views()
        task = _np(sa[3])
        assert np.array_equal(task, _np(sp[3])) and set(np.unique(task)) == {1, 2, 3, 4, 5}
        assert eu.same_bits(_np(sa[0]), _np(sp[0])) and eu.same_bits(_np(sa[1]), _np(sp[1]))
        assert (_np(sa[4]) == episode).all() and (_np(sp[4]) == episode).all()
