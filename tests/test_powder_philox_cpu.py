"""The host model of powderworld's Philox streams (tests/powder_philox_np.py)
is sound, and every scenario that tests/test_powder_philox_gpu.py replays on the
device would notice a wrong layout: Philox known answers, agreement with the
oracle's C Philox, distinct counters over an env-episode, uniform and
independent fields, the sensitivity of each scenario to three near-miss layouts
and the digests of the model's own trajectories."""

import hashlib
import os

import numpy as np
import pytest

import powder_philox_np as m
from oracle import locomaze as orc_loco

# the published Philox4x32-10 vectors (Random123 kat_vectors)
KAT = [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     'd16cfe09 94fdcceb 5001e420 24126ea1'),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert ' '.join(f'{int(v):08x}' for v in m.philox4x32(ctr, key)) == want
    # vectorised: the three at once
    got = m.philox4x32([c for c, _, _ in KAT], [k for _, k, _ in KAT])
    assert [' '.join(f'{int(v):08x}' for v in row) for row in got] == [w for _, _, w in KAT]


def test_philox_agrees_with_the_oracle():
    rng = np.random.RandomState(5)
    ctr = rng.randint(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    key = rng.randint(0, 2 ** 32, size=(300, 2), dtype=np.uint64)
    got = m.philox4x32(ctr, key)
    for i in range(300):
        ref = orc_loco.philox4x32(ctr[i].astype(np.uint32), int(key[i, 0]), int(key[i, 1]))
        assert np.array_equal(got[i], ref), i


def test_draw_reduction():
    w = int(m.philox4x32(m.draw_counter(2 ** 32 + 5, 3, 2), m.key(2 ** 40 + 9, m.TAG_RESET))[0])
    assert m.draw(2 ** 40 + 9, m.TAG_RESET, 2 ** 32 + 5, 3, 2, 8) == (w * 8) >> 32
    assert m.draw_counter(2 ** 32 + 5, 3, 2) == (5, 3, 2, 1)
    assert m.key(2 ** 40 + 9, m.TAG_ACTION) == (9, 0x100 ^ 0x50570002)


@pytest.mark.parametrize('H', [32, 64])
def test_counters_of_an_env_episode_are_distinct(H):
    """Every goal slot of the longest task, the start slot and the step slots
    0 .. max_episode_steps - 1: no (counter, key) of the fields occurs twice."""
    longest = max(len(s) for ne in (5, 8) for s in m.task_sequences(ne))
    assert longest == 184
    slots = [m.RAND_GOAL | q for q in range(longest)] + [m.RAND_START] + [m.RAND_STEP | t for t in range(500)]
    seed, env, ep = 2 ** 40 + 11, 2 ** 32 + 3, 7
    packed, keys = [], set()
    for s in slots:
        ctr, key = m.field_counters(seed, env, ep, s, H)
        assert (ctr[..., 1] == 3).all() and (ctr[..., 2] == ep).all() and (ctr[..., 3] == s).all()
        assert int(ctr[..., 0].max()) < 2 ** 32
        packed.append((ctr[..., 3] << np.uint64(32) | ctr[..., 0]).ravel())
        keys.add(key)
    packed = np.concatenate(packed)
    assert len(keys) == 1 and len(np.unique(packed)) == len(packed) == len(slots) * 3 * H * H // 4
    # the limit: the purpose is OR-ed in, so an index of 2^24 repeats index 0 and one of 2^25 changes the purpose
    assert m.RAND_GOAL | (1 << 24) == m.RAND_GOAL | 0 and m.RAND_GOAL | (1 << 25) == m.RAND_STEP | 0


def test_tags_keep_the_scalar_draws_apart_from_the_fields():
    for seed in (0, 11, 2 ** 64 - 1):
        k1 = [m.key(seed, t)[1] for t in (m.TAG_RESET, m.TAG_ACTION, m.TAG_RAND)]
        assert len(set(k1)) == 3
        # the env's high word goes into key word 0 of the fields: word 1, where the tag is, stays
        for env in (0, 2 ** 32, 2 ** 63):
            assert m.field_counters(seed, env, 1, m.RAND_START, 32)[1][1] == k1[2]
    # reset slots 0..3 and action slots 0..elapsed are distinct counters under their own keys
    assert len({m.draw_counter(5, 1, s) for s in range(500)}) == 500


def _within(count, n, p, what):
    sd = np.sqrt(n * p * (1 - p))
    assert abs(count - n * p) <= 5 * sd, f'{what}: {count} of {n}, expected {n * p:.0f} +- {sd:.0f}'


def test_fields_are_uniform_and_independent():
    """The categories the rules cut the fields into (sim.py: rm > 0.5; ri below
    0.02 / 0.05 / 0.2 / 0.3; re below 0.05 / 0.4) occur with their
    probabilities, each within 5 binomial standard deviations, over 64 slots at
    H = 64 (262,144 cells); so does the joint table of the rm bit against the re
    category."""
    F = np.float32
    f = np.stack([m.rand_fields(20261, 3, 2, m.RAND_STEP | t, 64) for t in range(64)], axis=1).reshape(3, -1)
    n = f.shape[1]
    assert n >= 200000 and f.dtype == np.float32 and f.min() >= 0 and f.max() < 1
    rm = f[0] > F(0.5)
    ri = (f[1] >= F(0.02)).astype(int) + (f[1] >= F(0.05)) + (f[1] >= F(0.2)) + (f[1] >= F(0.3))
    re = (f[2] >= F(0.05)).astype(int) + (f[2] >= F(0.4))
    _within(int(rm.sum()), n, 0.5, 'rm > 0.5')
    for c, p in enumerate((0.02, 0.03, 0.15, 0.10, 0.70)):
        _within(int((ri == c).sum()), n, p, f'ri category {c}')
    for c, p in enumerate((0.05, 0.35, 0.60)):
        _within(int((re == c).sum()), n, p, f're category {c}')
        for b in (0, 1):
            _within(int(((re == c) & (rm == b)).sum()), n, 0.5 * p, f'rm bit {b} with re category {c}')


def test_forward_full_cases_are_sensitive():
    for size in (32, 64):
        w = m.forward_worlds(size)
        for chained in (True, False):
            right = m.forward_full_model(w, m.SEED, 8, chained=chained)
            for name, layout in m.WRONG_LAYOUTS.items():
                wrong = m.forward_full_model(w, m.SEED, 8, layout, chained=chained)
                for e in range(len(w)):
                    assert not np.array_equal(right[e], wrong[e]), (size, chained, name, e)


@pytest.mark.parametrize('name', m.FIELD_SCENARIOS)
def test_scenario_is_sensitive(name):
    """Under each wrong layout every env's trajectory differs from the right
    model's in a compared observation."""
    for lname, layout in m.WRONG_LAYOUTS.items():
        for env in range(m.scenario(name).n):
            assert m.first_difference(name, layout, env) is not None, (lname, env)


@pytest.mark.parametrize('name', m.STEP_SCENARIOS + m.EASY_SCENARIOS)
def test_scenario_meets_every_draw(name):
    """Replacements at each stage and auto-resets occur; every env is truncated
    at least twice."""
    recs, envs = m.trajectory(name)
    for stage in range(3):
        assert sum(e.replaced[stage] for e in envs) >= 1, stage
    assert sum(e.auto_resets for e in envs) >= 1
    trunc = np.array([r.truncated for r in recs if isinstance(r, m.Step)])
    assert (trunc.sum(axis=0) >= 2).all()
    if 'mixed' in name:  # stages 0, 1 and 2 side by side
        assert any(set(r.stage) == {0, 1, 2} for r in recs if isinstance(r, m.Step))


def test_env64_scenario_replaces_at_every_stage():
    envs = m.trajectory('medium32_env64').envs
    assert [e.env for e in envs] == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    for stage in range(3):
        assert sum(e.replaced[stage] for e in envs) >= 1


@pytest.mark.parametrize('name', m.OWN_SCENARIOS)
def test_own_sequence_succeeds_and_goes_on(name):
    recs, envs = m.trajectory(name)
    steps = [r for r in recs if isinstance(r, m.Step)]
    t = m.success_step(name)
    assert [k for k, r in enumerate(steps) if r.terminated[0]] == [t]
    assert len(steps) == t + 13 and envs[0].auto_resets == 1 and envs[0].episode == 2 and envs[0].elapsed == 12
    # the step that terminates returns the next episode's first observation: stage 0, empty action frame
    assert not steps[t].obs[0][..., 3:].any()


def _digest(name):
    h = hashlib.sha256()
    for r in m.trajectory(name).records:
        for i, ob in enumerate(r.obs):
            if ob is None:
                continue
            h.update(np.ascontiguousarray(ob).tobytes())
            if isinstance(r, m.Reset):
                h.update(np.ascontiguousarray(r.goal[i]).tobytes())
            else:
                h.update(bytes([int(r.terminated[i]), int(r.truncated[i])]))
    return h.hexdigest()[:16]


# Digests of the model's own trajectories: a slip in the model (two channels
# swapped, elapsed + 1 as the step slot) shows here before any device is asked.
# They come from the model as documented, never from a device; re-record with
# OGBX_WRITE_PHILOX_DIGESTS=1 (prints the table) after a deliberate change of a
# scenario.
DIGESTS = {
    'medium32': '5875371fb7c37caf',
    'hard32': 'ad44de665845b6af',
    'medium64': '25f09cc79ee22dd6',
    'medium32_mixed': '3166a691927480ed',
    'hard32_mixed': 'b7785eb5fbcf6d09',
    'medium32_env64': '1c0a6cb905e772e8',
    'reset_medium_given': '4612278adae53c3d',
    'reset_medium_drawn': '494ad7531a9dcd18',
    'reset_hard_given': 'cad23983bcad552d',
    'reset_hard_drawn': '847ca3fb76badf7f',
    'medium32_task3': '923d660b2f668403',
    'hard32_task4': 'aa3769775d303f2a',
    'easy32': 'bc52d6a18d9bafa7',
    'easy64': 'ec517d4e2ec5585a',
    'easy32_task1': '793c6afeb7831d65',
    'easy64_task3': '43d98e9c96170df5',
    'reset_easy_given': '8278cbff3f1778cb',
    'reset_easy_drawn': 'eab2e20227507b5a',
}


@pytest.mark.parametrize('name', m.FIELD_SCENARIOS + m.EASY_SCENARIOS + [s for s in m.OWN_SCENARIOS if 'easy' in s]
                         + [s for s in m.RESET_SCENARIOS if 'easy' in s])
def test_model_trajectory_digest(name):
    d = _digest(name)
    if os.environ.get('OGBX_WRITE_PHILOX_DIGESTS'):
        print(f"    '{name}': '{d}',")
        return
    assert d == DIGESTS[name]
