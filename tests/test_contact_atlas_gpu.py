"""GPU: the pointmaze contact step on the contact-regime atlas
(tests/contact_atlas.py, certified by tests/test_contact_atlas_cpu.py): states
placed in the impedance band, on cell edges, at wall ends, in corners, at rest
against a wall, within an ulp of the contact thresholds, inside wall cells and
off the map -- the regimes that uniform draws over a free cell reach only by
luck.  Against the oracle at 1e-9 and the enumeration model at 1e-10, the
tolerances of tests/test_locomaze_gpu.py and tests/test_contact_pin_gpu.py.
"""

import numpy as np
import pytest
import torch

import contact_atlas as ca
import ogbench_amd
from ogbench_amd import _lib
from oracle import locomaze as orc
from test_contact_pin import TOL_MODEL

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _physics(gpu, maze, q, a=None):
    env = ogbench_amd.MazeEnv('point', maze, num_envs=1, device=gpu)
    a = np.zeros_like(q) if a is None else a
    out, contact = env.physics(torch.tensor(np.array(q)), torch.tensor(np.array(a)))
    out, contact = out.cpu().numpy(), contact.cpu().numpy()
    env.close()
    return out, contact


def _check_against_oracle(maze, q, a, got, contact):
    ref, rc = orc.physics(maze, q, a)
    assert np.array_equal(contact, rc)
    assert np.isfinite(got).all()
    assert np.array_equal(got[rc == 0], ref[rc == 0])
    err = np.abs(got - ref).max()
    print(f'max |kernel - oracle| = {err:.3g} over {len(q)} states, {int(rc.sum())} in contact')
    assert err <= TOL, err
    return rc


_CASES = [(label, maze) for label in ca.CLASSES for maze in ca.MAZES
          if label != 'in_wall_corner' or maze in ca.IN_WALL_CORNER_MAZES]


@pytest.mark.parametrize('label,maze', _CASES, ids=[f'{label}-{maze}' for label, maze in _CASES])
def test_class_matches_oracle_and_model(gpu, label, maze):
    """env.physics with zero f64 actions on one class: contact flags equal to
    the oracle's, flag-0 lanes returned bit-identical, contact lanes within
    1e-9 of the oracle and, where the enumeration model has an answer, within
    1e-10 of it.

    Measured on an MI355X: the worst |kernel - oracle| is 1.4e-14 and the
    worst |kernel - model| 1.8e-13 (edge_wall_end, where the oracle is as far
    from the model).  in_wall_cell of medium holds the state (9.909, -1.609):
    inside a wall cell within the radius of a corner where four wall cells
    meet, it touches its own box, both side boxes and the diagonal one; with
    three generic slots the kernel was 0.0341 off there (point_step_walled,
    point_contact.h, holds the fourth)."""
    q = ca.states(maze, label)
    a = np.zeros_like(q)
    got, contact = _physics(gpu, maze, q, a)
    rc = _check_against_oracle(maze, q, a, got, contact)
    assert np.array_equal(got[rc == 0], q[rc == 0])
    if label in ca.MODEL_CLASSES:
        sub = ca.model_subset(maze, label)
        assert rc[sub].all()
        err = np.abs(got[sub] - ca.model_answers(maze, label)).max()
        print(f'max |kernel - model| = {err:.3g} over {len(sub)} states')
        assert err <= TOL_MODEL, err


@pytest.mark.parametrize('maze', ca.MAZES)
def test_edge_wall_end_is_continuous_across_the_cell_edge(gpu, maze):
    """One box seen as a corner slot (2 - 1e-9), by the generic collider (2.0)
    and as a face slot (2 + 1e-9): the three outputs differ from each other by
    no more than the model's own outputs for the triple do, plus 2 TOL_MODEL."""
    q = ca.edge_wall_end(maze)
    assert np.array_equal(ca.model_subset(maze, 'edge_wall_end'), np.arange(len(q)))
    shape = (-1, len(ca.EDGE_PEN), len(ca.EDGE_E), 2)
    got = _physics(gpu, maze, q)[0].reshape(shape)
    exp = ca.model_answers(maze, 'edge_wall_end').reshape(shape)
    k = [ca.EDGE_E.index(e) for e in (-1e-9, 0.0, 1e-9)]
    worst = 0.0
    for a, b in ((k[0], k[1]), (k[1], k[2]), (k[0], k[2])):
        dg = np.abs(got[:, :, a] - got[:, :, b]).max(-1)
        de = np.abs(exp[:, :, a] - exp[:, :, b]).max(-1)
        worst = max(worst, float((dg - de).max()))
        assert (dg <= de + 2 * TOL_MODEL).all(), (a, b, float((dg - de).max()))
    print(f'max (kernel difference - model difference) = {worst:.3g}')


@pytest.mark.parametrize('maze', ca.MAZES)
@pytest.mark.parametrize('f64', [False, True])
def test_rest_with_small_actions(gpu, f64, maze):
    """Resting states with the small action into the wall that their
    trajectories held (|a| <= 0.01: the step's 0.2 a lands inside the band),
    and with its opposite, as float32 and float64 actions, against the oracle."""
    q = ca.rest(maze)
    press = ca.rest_press(maze)
    q = np.concatenate([q, q])
    a = np.concatenate([press, -press]).astype(np.float64 if f64 else np.float32)
    got, contact = _physics(gpu, maze, q, a)
    rc = _check_against_oracle(maze, q, a, got, contact)
    assert rc[:len(press)].mean() > 0.9


def _whole_atlas(maze):
    q = np.concatenate([ca.states(maze, label) for label in ca.CLASSES])
    if len(q) % 64 == 0:
        q = q[:-1]
    return q


@pytest.mark.parametrize('maze', ca.MAZES)
def test_whole_atlas_through_step_and_rollout(gpu, maze):
    """Every class restored with load_state_dict (goal far away, no
    auto-reset, N no multiple of 64) and stepped twice: env.step (the plain
    single-step instantiation), ogbx_maze_step with k_steps = 1 at 32 envs per
    wave (generic) and one rollout launch (generic, K = 2) agree bit for bit,
    and equal the oracle to 1e-9.

    Measured on an MI355X: the three paths agree bit for bit in every maze,
    1.4e-14 from the oracle."""
    q = _whole_atlas(maze)
    n, K = len(q), 2
    assert n % 64 != 0
    acts = torch.zeros(K, n, 2, dtype=torch.float64, device=gpu)
    envs = [ogbench_amd.MazeEnv('point', maze, num_envs=n, device=gpu, auto_reset=False) for _ in range(3)]
    for e in envs:
        e.reset(seed=1, options=dict(task_id=1))
        sd = e.state_dict()
        sd['qpos'] = torch.tensor(q, device=gpu)
        sd['goal'] = torch.full((n, 2), -5e4, dtype=torch.float64, device=gpu)
        sd['elapsed'].zero_()
        e.load_state_dict(sd)
    st = dict(qpos=q.copy(), goal=sd['goal'].cpu().numpy().copy(), elapsed=sd['elapsed'].cpu().numpy().copy(),
              task=sd['task'].cpu().numpy().copy(), episode=sd['episode'].cpu().numpy().view(np.uint32).copy(),
              opts=orc._opts())
    ref = orc.step(maze, st, acts.cpu().numpy(), nthreads=8)
    plain = []
    for t in range(K):
        ob, rew, term, trunc, info = envs[0].step(acts[t])
        assert not term.any() and not trunc.any() and not info['success'].any()
        plain.append(ob.cpu().numpy().copy())
    plain = np.stack(plain)
    _lib.check(envs[1]._L.ogbx_maze_set_envs_per_wave(envs[1]._h, 32))
    generic = np.stack([envs[1].rollout(acts[t:t + 1])['obs'].cpu().numpy()[0].copy() for t in range(K)])
    roll = envs[2].rollout(acts)
    assert np.array_equal(plain, generic)
    assert np.array_equal(plain, roll['obs'].cpu().numpy())
    assert not roll['terminated'].any() and not roll['truncated'].any()
    for e in envs:
        assert np.array_equal(e.get_xy().cpu().numpy(), plain[-1])
    assert np.isfinite(plain).all()
    err = np.abs(plain - ref['obs']).max(axis=(1, 2))
    print(f'max |step - oracle| per step = {err}')
    assert err.max() <= TOL, err
    _, rc = orc.physics(maze, q, np.zeros_like(q))
    assert np.array_equal(plain[0][rc == 0], q[rc == 0])  # free lanes, zero action: the state unchanged
    for e in envs:
        e.close()


def _wave_independence(gpu, maze):
    per = 48
    parts = []
    for label in ca.CLASSES:
        q = ca.states(maze, label)
        if len(q) == 0:
            assert label == 'in_wall_corner' and maze not in ca.IN_WALL_CORNER_MAZES
            continue
        parts.append(q[np.unique(np.linspace(0, len(q) - 1, per).round().astype(int))])
    grouped = np.concatenate(parts)
    cls = np.concatenate([np.full(len(p), c) for c, p in enumerate(parts)])
    rank = np.concatenate([np.arange(len(p)) for p in parts])
    order = np.lexsort((cls, rank))  # round robin over the classes
    n = len(grouped)
    assert len(set(cls[order][:len(parts)].tolist())) == len(parts)  # a wave's first lanes: one of each class
    solo = np.zeros((n * 64, 2))
    solo[::64] = grouped
    _, rc0 = orc.physics(maze, np.zeros((1, 2)), np.zeros((1, 2)))
    assert rc0[0] == 0  # the padding lanes are free
    out_g, c_g = _physics(gpu, maze, grouped)
    out_i, c_i = _physics(gpu, maze, grouped[order])
    out_s, c_s = _physics(gpu, maze, solo)
    assert np.array_equal(out_i, out_g[order]) and np.array_equal(c_i, c_g[order])
    assert np.array_equal(out_s[::64], out_g) and np.array_equal(c_s[::64], c_g)
    pad = np.ones(n * 64, bool)
    pad[::64] = False
    assert not c_s[pad].any() and not out_s[pad].any()
    assert 0.5 < c_g.mean() < 1.0


def test_results_do_not_depend_on_the_regimes_sharing_a_wave(gpu):
    """States of every class interleaved lane by lane within each 64-lane
    wave, the same states grouped class by class, and each state alone in a
    wave padded with 63 free lanes ([0, 0] of pointmaze-large): bit-identical
    outputs and flags.  Extends the wavefront-composition guarantee of
    tests/test_locomaze_gpu.py to band, on-edge, in-wall and off-map lanes."""
    _wave_independence(gpu, 'large')


def test_four_contact_lanes_do_not_depend_on_their_wave(gpu):
    """The same in pointmaze-medium, whose atlas holds the four-contact
    in-wall lanes (in_wall_corner; large has no site for them): 48 of them
    interleaved with every other class, grouped, and alone in a wave."""
    assert 'medium' in ca.IN_WALL_CORNER_MAZES
    _wave_independence(gpu, 'medium')
