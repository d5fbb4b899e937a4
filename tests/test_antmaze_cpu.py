"""CPU: the antmaze wrapper oracle (oracle/antmaze_np.py) pinned against the
fixture tests/golden/antmaze_golden.npz, generated from the reference's own
MazeEnv/AntEnv methods by make_golden_ant.py: reset ob and goal from the
recorded draws, then 40 wrapper steps on given post-physics states (ob,
success with the fma-rounded 2-norm, terminated, reward, TimeLimit) for
success_timing 'post' and 'pre'.  The GPU kernel is held to the same fixture
in tests/test_antmaze_gpu.py."""

import os

import numpy as np
import pytest

from oracle import antmaze_np as am

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'antmaze_golden.npz')


@pytest.mark.parametrize('timing', ['post', 'pre'])
def test_oracle_matches_reference_fixture(timing):
    d = np.load(GOLDEN)
    g = {k[len(timing) + 1:]: d[k] for k in d.files if k.startswith(timing + '_')}
    ob0, goal = am.reset_obs(g['task'], g['noise'], g['body_draws'])
    assert np.array_equal(ob0, g['reset_obs'])
    assert np.array_equal(goal, g['reset_goal'])
    assert np.array_equal(am.goal_obs(goal, g['goal_states']), g['reset_goal_ob'])
    b = am.Batch(g['task'], g['noise'], g['body_draws'], max_steps=int(d['max_episode_steps']), timing=timing)
    for k in range(g['obs'].shape[0]):
        obs, rew, term, trunc, succ = b.step(g['qpos_post'][k], g['qvel_post'][k])
        assert np.array_equal(obs, g['obs'][k])
        assert np.array_equal(succ, g['success'][k].astype(bool))
        assert np.array_equal(term, g['terminated'][k].astype(bool))
        assert np.array_equal(trunc, g['truncated'][k].astype(bool))
        assert np.array_equal(rew, g['reward'][k])
    assert g['success'].sum() > 50


def test_within_decides_boundary_exactly():
    # pairs whose plain sum and fma-rounded sum fall on opposite sides of 0.5
    rng = np.random.RandomState(0)
    ang = rng.uniform(0, 2 * np.pi, 20000)
    r = 0.5 + rng.normal(0, 1, 20000) * 1e-16
    dx, dy = r * np.cos(ang), r * np.sin(ang)
    from fractions import Fraction

    exact = np.array([np.sqrt(float(Fraction(float(y)) ** 2 + Fraction(float(x * x)))) <= 0.5
                      for x, y in zip(dx, dy)])
    assert np.array_equal(am.within(dx, dy), exact)


# ---- tests/golden/antmaze_edges_golden.npz (make_golden_ant_edges.py): the
# wrapper's edges -- success rounding on the circle, teleport, configurations,
# the host loop's episodes -- in blocks of 70 envs.

import antmaze_edges_util as eu  # noqa: E402
from oracle import locomaze as orc  # noqa: E402


@pytest.mark.parametrize('timing', eu.TIMINGS)
@pytest.mark.parametrize('name', eu.BLOCKS)
def test_oracle_reproduces_edges_fixture(name, timing):
    """The restatement gives every block bit for bit: reset ob / goal / goal
    observation, then per step ob, reward, flags, the body state (teleports
    and the loop's resets included) and the final observation."""
    g = eu.block(name, timing)
    b = eu.oracle_batch(name, timing, g)
    assert eu.same_bits(b.reset_ob, g['reset_obs'])
    assert eu.same_bits(b.goal, g['reset_goal'])
    assert eu.same_bits(am.goal_obs(b.goal, g['goal_states']), g['reset_goal_ob'])
    for t in range(g['obs'].shape[0]):
        obs, rew, term, trunc, succ = eu.oracle_step(name, b, g, t)
        assert eu.same_bits(obs, g['obs'][t]), t
        assert eu.same_bits(rew, g['reward'][t]), t
        assert np.array_equal(succ, g['success'][t].astype(bool)), t
        assert np.array_equal(term, g['terminated'][t].astype(bool)), t
        assert np.array_equal(trunc, g['truncated'][t].astype(bool)), t
        assert eu.same_bits(b.body_q, g['body_qpos'][t]) and eu.same_bits(b.body_v, g['body_qvel'][t]), t
        assert eu.same_bits(b.xy, g['body_qpos'][t][:, :2]), t
        if name == 'ep':
            assert eu.same_bits(b.final_obs, g['final_obs'][t]), t


def _plain(dx, dy, tol):
    return np.sqrt(dx * dx + dy * dy) <= tol


def test_edges_fixture_circle_rows_reach_the_rational_branch():
    """Class (a): the fma and the plain rounding disagree, both outcomes, and
    `within` (through its rational branch) gives the reference's verdict;
    class (b): distance exactly 0.5 succeeds, an ulp outward fails; class (c):
    NaN / inf rows never succeed and are copied to obs."""
    kinds = eu.load()['edge_class']
    for timing, row in (('post', 0), ('pre', 1)):
        g = eu.block('edge', timing)
        verdict = g['success'][row].astype(bool)
        assert not g['success'][1 - row].any()
        xy, goal = g['qpos_post'][0][:, :2], g['reset_goal']
        dx, dy = xy[:, 0] - goal[:, 0], xy[:, 1] - goal[:, 1]
        a = kinds == eu.EDGE_A
        assert a.sum() >= 16 and verdict[a].sum() >= 4 and (~verdict[a]).sum() >= 4
        with np.errstate(invalid='ignore'):
            near = np.abs(np.sqrt(dx * dx + dy * dy) - 0.5) <= 1e-12
        assert near[a].all() and np.array_equal(_plain(dx[a], dy[a], 0.5), ~verdict[a])
        assert np.array_equal(am.within(dx, dy)[a], verdict[a])
        b = kinds == eu.EDGE_B
        assert b.sum() == 12 and near[b].all() and not (goal[b] % 1).any()
        r = np.maximum(np.abs(dx[b]), np.abs(dy[b]))
        assert (r == 0.5).sum() == 4 and (r > 0.5).sum() == 4 and (r < 0.5).sum() == 4
        assert np.array_equal(verdict[b], r <= 0.5)
        c = kinds == eu.EDGE_C
        assert c.sum() >= 8 and not np.isfinite(xy[c]).all(1).any() and not verdict[c].any()
        assert np.isnan(xy[c]).any() and np.isposinf(xy[c]).any() and np.isneginf(xy[c]).any()
        assert eu.same_bits(g['obs'][0][:, :2], xy)


def test_edges_fixture_promises():
    d = eu.load()
    assert os.path.getsize(eu.EDGES) <= 1_000_000
    ins, outs, radius = am.teleport_table(eu.teleport_info())
    for timing in eu.TIMINGS:
        for name in eu.BLOCKS:
            g = eu.block(name, timing)
            assert g['task'].shape == (eu.N,) and g['obs'].shape[1:] == (eu.N, 29)
        for name in ('cfg1', 'cfg2'):
            g = eu.block(name, timing)
            assert g['obs'].shape[0] == 12 and int(g['max_steps']) == 8
            assert g['success'].sum() >= 40 and g['truncated'].sum() >= 70
        assert eu.block('cfg1', timing)['terminated'].sum() == 0
        g = eu.block('cfg2', timing)
        assert set(np.unique(g['reward'])) == {-1.0, 0.0} and (g['task'] != 3).sum() > 40
        # tp: both in-portals entered, every out-portal drawn, circle rows of both outcomes
        g = eu.block('tp', timing)
        T = g['obs'].shape[0]
        assert T == 16
        moved = (g['body_qpos'][:, :, :2] != g['qpos_post'][:, :, :2]).any(2)
        portal = np.abs(g['qpos_post'][:, :, None, :2] - ins).sum(3).argmin(2)
        for p in range(len(ins)):
            assert (moved & (portal == p)).any(0).sum() >= 10
        used = g['tp_draws'][moved]
        assert all((used == o).sum() >= 5 for o in range(len(outs)))
        circ = g['tp_circle'].astype(bool)
        assert circ.sum() >= 8 and 0 < moved[circ].sum() < circ.sum()
        xy = g['qpos_post'][circ][:, :2]
        c = ins[portal[circ]]
        assert np.array_equal(_plain(xy[:, 0] - c[:, 0], xy[:, 1] - c[:, 1], 1.5 * radius), ~moved[circ])
        if timing == 'pre':  # the step after a teleport onto the goal's out-portal succeeds
            after = moved[:-1] & g['success'][1:].astype(bool) & (g['task'] == 0)
            assert after.sum() >= 10
        # ep: the host loop's episodes
        g = eu.block('ep', timing)
        ends = (g['terminated'] | g['truncated']).astype(bool)
        assert g['obs'].shape[0] == 28 and int(g['max_steps']) == 7
        assert ends.sum(0).min() >= 3 and g['terminated'].sum() >= 60 and g['truncated'].sum() >= 100
        assert (g['terminated'] & g['truncated']).sum() >= 4 and ends[:, 64:].any()
        assert np.array_equal(~np.isnan(g['reset_states'][:, :, 0]), ends)
    assert d['src_sha256'].size >= 14


def test_edges_fixture_philox_draws_are_current():
    """The stored teleport indices and auto-reset draws are what libogbx's
    Philox layout gives for the stored seed: a change of that layout shows up
    here, as a stale fixture, before any parity test."""
    for timing in eu.TIMINGS:
        g = eu.block('tp', timing)
        seed = int(g['seed'])
        exp = np.array([[eu.teleport_index(seed, i, 1, t) for i in range(eu.N)] for t in range(g['obs'].shape[0])])
        assert np.array_equal(g['tp_draws'], exp), 'stale fixture: teleport draws (regenerate antmaze_edges_golden.npz)'
        g = eu.block('ep', timing)
        seed = int(g['seed'])
        ends = (g['terminated'] | g['truncated']).astype(bool)
        first = np.stack([orc.reset_draws(1, seed, env_base=i, episode=1)[0] for i in range(eu.N)])
        assert eu.same_bits(g['noise'], first), 'stale fixture: reset draws (regenerate antmaze_edges_golden.npz)'
        for i in range(eu.N):
            e = 1
            for t in np.nonzero(ends[:, i])[0]:
                e += 1
                assert eu.same_bits(g['reset_noise'][t, i], orc.reset_draws(1, seed, env_base=i, episode=e)[0]), \
                    'stale fixture: auto-reset draws (regenerate antmaze_edges_golden.npz)'
