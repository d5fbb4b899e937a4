"""The powderworld kernels on their Philox path (no rand=, draws= or
reset_action= anywhere) equal the host model of the documented stream layout
(tests/powder_philox_np.py around the NumPy oracles), bit for bit: resets with
a given and a drawn task, single steps in and out of phase with invalid actions
at every stage and auto-resets, the fused rollout, success inside a run, env
indices on both sides of 2^32, W = 64, the easy kernels, and forward_full
without rand.  tests/test_powder_philox_cpu.py shows that each scenario here
would notice a rotated channel, a slot off by one or a wrong row mapping."""

import numpy as np
import pytest
import torch

import ogbench_amd
import powder_philox_np as m
from ogbench_amd import _lib

pytestmark = pytest.mark.gpu


def _make(gpu, sc):
    return ogbench_amd.make(f'powderworld-{sc.env_type}-v0', num_envs=sc.n, device=gpu, world_size=sc.size,
                            max_episode_steps=sc.max_episode_steps, auto_reset=sc.auto_reset, env_base=sc.env_base)


def _np(t):
    return t.cpu().numpy()


def _check_reset(env, op, rec):
    _, seed, tasks, mask = op
    options = {} if tasks is None else dict(task_id=torch.tensor(tasks, dtype=torch.int32))
    ob, info = env.reset(seed=seed, options=options, mask=None if mask is None else torch.tensor(mask, dtype=torch.uint8))
    ob, goal = _np(ob), _np(info['goal'])
    for i in range(env.num_envs):
        if rec.obs[i] is not None:
            assert np.array_equal(ob[i], rec.obs[i]), ('reset obs', i)
            assert np.array_equal(goal[i], rec.goal[i]), ('reset goal obs', i)


def _check_step(t, i_envs, got, rec):
    """got: (obs, reward, terminated, truncated, success) arrays [n, ...] of step t."""
    for k, what in enumerate(('obs', 'reward', 'terminated', 'truncated', 'success')):
        want = rec[k]
        for i in i_envs:
            assert np.array_equal(got[k][i], want[i]), (what, 'step', t, 'env', i)


def _check_final(env, envs):
    n = env.num_envs
    sd = env.state_dict()
    world = _np(env.world_full()) if envs[0].full else _np(sd['world'])
    goal = _np(env.goal_ids())
    for i, e in enumerate(envs):
        assert np.array_equal(world[i], e.world()), ('world', i)
        assert np.array_equal(goal[i], e.goal_ids()), ('goal ids', i)
    assert np.array_equal(_np(env.cur_task_ids), [e.task for e in envs])
    assert np.array_equal(_np(sd['ctrl']), np.array([e.ctrl for e in envs], np.int32))
    assert np.array_equal(_np(sd['elapsed']), np.array([e.elapsed for e in envs], np.int32))
    assert np.array_equal(_np(sd['episode']), np.array([e.episode for e in envs], np.int32))
    assert n == len(envs)


def _replay_single_steps(gpu, name):
    sc = m.scenario(name)
    recs, envs = m.trajectory(name)
    env = _make(gpu, sc)
    recs = iter(recs)
    t = 0
    for op in sc.program:
        if op[0] == 'reset':
            _check_reset(env, op, next(recs))
        elif op[0] == 'phase':
            env.set_step_phase(op[1])
        else:
            ob, rew, term, trunc, info = env.step(np.array(op[1], np.int64))
            _check_step(t, range(sc.n), [_np(v) for v in (ob, rew, term, trunc, info['success'])], next(recs))
            t += 1
    _check_final(env, envs)
    env.close()
    return t


def _replay_fused(gpu, name):
    """Reset, then every step of the scenario in one launch."""
    sc = m.scenario(name)
    recs, envs = m.trajectory(name)
    assert [op[0] for op in sc.program] == ['reset'] + ['step'] * (len(sc.program) - 1)
    env = _make(gpu, sc)
    _check_reset(env, sc.program[0], recs[0])
    out = env.rollout(np.array([op[1] for op in sc.program[1:]], np.int64))
    got = [_np(out[k]) for k in ('obs', 'reward', 'terminated', 'truncated', 'success')]
    for t, rec in enumerate(recs[1:]):
        _check_step(t, range(sc.n), [g[t] for g in got[:2]] + [g[t].astype(bool) for g in got[2:]], rec)
    _check_final(env, envs)
    env.close()


@pytest.mark.parametrize('size', [32, 64])
def test_forward_full_without_rand(gpu, size):
    """Hard worlds holding every element: 8 chained forwards (slot (3<<24) | q)
    and 8 single calls (slot (3<<24) | 0 each) under env = world index, episode
    0 and the key of the handle's seed -- which a reset or ogbx_powder_set_seed
    sets (0 on a fresh handle): set here explicitly."""
    w = m.forward_worlds(size)
    env = ogbench_amd.make('powderworld-hard-v0', num_envs=1, device=gpu, world_size=size)
    _lib.check(env._L.ogbx_powder_set_seed(env._h, m.SEED))
    got = _np(env.forward_full(w, 8))
    assert np.array_equal(got, m.forward_full_model(w, m.SEED, 8))
    cur = torch.as_tensor(w)
    for _ in range(8):
        cur = env.forward_full(cur, 1)
    assert np.array_equal(_np(cur), m.forward_full_model(w, m.SEED, 8, chained=False))
    env.close()


@pytest.mark.parametrize('name', m.RESET_SCENARIOS)
def test_reset(gpu, name):
    """First observation, info['goal'], goal ids, task ids (given, or drawn at
    slot 0) and the state of 6 envs after one reset."""
    sc = m.scenario(name)
    recs, envs = m.trajectory(name)
    env = _make(gpu, sc)
    _check_reset(env, sc.program[0], recs[0])
    _check_final(env, envs)
    env.close()


def _assert_every_draw_occurs(name):
    """From the model: replacements at stages 0, 1 and 2 (the light kernel's
    draw and the full kernel's) and auto-resets (the in-kernel goal replay)."""
    envs = m.trajectory(name).envs
    for stage in range(3):
        assert sum(e.replaced[stage] for e in envs) >= 1, stage
    assert min(e.auto_resets for e in envs) >= 2


@pytest.mark.parametrize('name', ['medium32', 'hard32', 'medium64'])
def test_single_steps_in_phase(gpu, name):
    _assert_every_draw_occurs(name)
    assert _replay_single_steps(gpu, name) == 15


@pytest.mark.parametrize('name', ['medium32_mixed', 'hard32_mixed'])
def test_single_steps_out_of_phase(gpu, name):
    """Stages 0, 1 and 2 side by side after masked re-resets (the sparse and the
    light kernel in one step), one wrong set_step_phase hint on the way."""
    assert any(op[0] == 'phase' for op in m.scenario(name).program)
    _assert_every_draw_occurs(name)
    assert any(set(r.stage) == {0, 1, 2} for r in m.trajectory(name).records if isinstance(r, m.Step))
    _replay_single_steps(gpu, name)


@pytest.mark.parametrize('name', ['medium32', 'hard32'])
def test_fused_rollout(gpu, name):
    _replay_fused(gpu, name)


@pytest.mark.parametrize('name', ['medium32_task3', 'hard32_task4'])
def test_success_inside_a_philox_run(gpu, name):
    """The env plays its task's own sequence: terminated at the model's step,
    whose observation is the next episode's first; 12 more steps follow."""
    steps = [r for r in m.trajectory(name).records if isinstance(r, m.Step)]
    assert [t for t, r in enumerate(steps) if r.terminated[0]] == [m.success_step(name)]
    assert _replay_single_steps(gpu, name) == m.success_step(name) + 13


def test_env_index_above_32_bits(gpu):
    """env_base = 2^32 - 2: two envs on either side of the boundary (the field
    key's xor with the high word, word 3 of the draw counter)."""
    assert m.scenario('medium32_env64').env_base == 2 ** 32 - 2
    assert _replay_single_steps(gpu, 'medium32_env64') == 12


@pytest.mark.parametrize('name', ['easy32', 'easy64'])
def test_easy_steps_and_rollout(gpu, name):
    _assert_every_draw_occurs(name)
    assert _replay_single_steps(gpu, name) == 30
    _replay_fused(gpu, name)


@pytest.mark.parametrize('name', ['easy32_task1', 'easy64_task3'])
def test_easy_success(gpu, name):
    assert _replay_single_steps(gpu, name) == m.success_step(name) + 13
