"""CPU checks of the play policy's action plan: the NumPy restatement
(tests/play_np.py) against the reference's recorded draws and actions
(tests/golden/play_golden.npz), its closed-form sequences against list-built
ones, and the host argument checks."""

import itertools
import os

import numpy as np
import pytest

import play_np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'play_golden.npz')
CASES = 'abcde'


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.mark.parametrize('case', CASES)
def test_play_np_replays_the_reference(gold, case):
    E, T, ne, world = (int(v) for v in gold[f'{case}_meta'])
    p = float(gold[f'{case}_p_random'])
    acts = gold[f'{case}_actions'].reshape(E, T)
    for e in range(E):
        n = int(gold[f'{case}_tape_len'][e])
        a, used, _ = play_np.plan_episode(gold[f'{case}_tape'][e, :n], T, world // 4, ne, p)
        assert used == n
        assert np.array_equal(a, acts[e])


def test_fixture_cases_are_the_issue_s(gold):
    want = dict(a=(2, 61, 2, 0.5), b=(2, 31, 5, 0.5), c=(2, 31, 8, 0.5), d=(8, 1001, 2, 0.5), e=(8, 1001, 2, 0.0))
    for case, (E, T, ne, p) in want.items():
        assert tuple(gold[f'{case}_meta'][:3]) == (E, T, ne) and float(gold[f'{case}_p_random']) == p
    for case in 'abc':
        E, T = want[case][:2]
        assert gold[f'{case}_obs'].shape == (E * T, 32, 32, 6)
        term = gold[f'{case}_terminals'].reshape(E, T)
        assert term[:, -1].all() and not term[:, :-1].any()
    assert gold['b_rand'].shape == gold['c_rand'].shape == (2, 10, 3, 32, 32)


def test_fisher_yates_round_trips_all_24_orders():
    seen = set()
    for j3, j2, j1 in itertools.product(range(4), range(3), range(2)):
        perm = play_np.perm_from_js(j3, j2, j1)
        assert play_np.js_from_perm(perm) == (j3, j2, j1)
        seen.add(tuple(perm))
    assert seen == set(itertools.permutations(range(4)))
    # and it is what a top-down Fisher-Yates does to a list
    for j3, j2, j1 in itertools.product(range(4), range(3), range(2)):
        x = list('abcd')
        for i, j in ((3, j3), (2, j2), (1, j1)):
            x[i], x[j] = x[j], x[i]
        assert x == [['a', 'b', 'c', 'd'][k] for k in play_np.perm_from_js(j3, j2, j1)]


SIZE = 8


def test_fill_closed_form_equals_the_list():
    for fx, fy, fxy in itertools.product((0, 1), repeat=3):
        seq = []
        for i in range(SIZE * SIZE):
            x, y = i % SIZE, i // SIZE
            x = SIZE - x - 1 if fx else x
            y = SIZE - y - 1 if fy else y
            if fxy:
                x, y = y, x
            seq.append((x, y))
        assert [play_np.fill_entry(i, SIZE, fx, fy, fxy) for i in range(SIZE * SIZE)] == seq
        assert sorted(seq) == sorted(itertools.product(range(SIZE), repeat=2))


def test_line_closed_form_equals_the_list():
    for target, fd, fxy in itertools.product(range(SIZE), (0, 1), (0, 1)):
        seq = []
        for i in range(SIZE):
            x, y = i, target
            y = SIZE - 1 - y if fd else y
            if fxy:
                x, y = y, x
            seq.append((x, y))
        assert [play_np.line_entry(i, SIZE, target, fd, fxy) for i in range(SIZE)] == seq


def test_square_closed_form_equals_the_list():
    perms = [play_np.perm_from_js(*js) for js in itertools.product(range(4), range(3), range(2))]
    n = 0
    for length in range(1, SIZE):
        for x1, y1 in itertools.product(range(SIZE - length), repeat=2):
            x2, y2 = x1 + length, y1 + length
            for rev in range(16):
                sides = [[(x1, y) for y in range(y1, y2 + 1)], [(x2, y) for y in range(y1, y2 + 1)],
                         [(x, y1) for x in range(x1, x2 + 1)], [(x, y2) for x in range(x1, x2 + 1)]]
                for k in range(4):
                    if (rev >> k) & 1:
                        sides[k].reverse()
                perm = perms[n % 24]  # every order, cycled over the cases
                n += 1
                seq = [xy for k in perm for xy in sides[k]]
                got = [play_np.square_entry(s, length, x1, y1, rev, perm) for s in range(4 * (length + 1))]
                assert got == seq
                assert all(0 <= x < SIZE and 0 <= y < SIZE for x, y in got)


def test_behavior_cdf_is_numpy_s():
    from ogbench_amd import _play

    p = np.array([1, 3, 3]) / 7
    cdf = p.cumsum()
    cdf /= cdf[-1]
    assert np.array_equal(_play.behavior_cdf(), cdf) and _play.behavior_cdf()[-1] == 1.0
    assert np.array_equal(play_np.behavior_cdf(), cdf)
    with pytest.raises(ValueError):
        _play.behavior_cdf((1, -1, 3))


def test_play_header_version_matches_the_binding():
    import re

    from ogbench_amd import _lib, _play

    text = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), 'ogbx_play.h')).read()
    assert int(re.search(r'#define\s+OGBX_PLAY_API_VERSION\s+(\d+)', text).group(1)) == _play.PLAY_API_VERSION
    assert int(re.search(r'#define\s+OGBX_POWDER_MODE_DATA\s+(\d+)', text).group(1)) == _play.POWDER_MODE_DATA
    L = _play.bind()
    assert L.ogbx_play_api_version() == _play.PLAY_API_VERSION
    for name in ('ogbx_play_powder_reset', 'ogbx_play_plan', 'ogbx_play_sample_semantic'):
        assert hasattr(L, name)


def test_play_entry_points_validate_before_device_work():
    """NULL pointers and bad sizes are OGBX_EINVAL without touching a device."""
    from ogbench_amd import _lib, _play

    L = _play.bind()
    cfg = _play.PlayConfig(size=8, num_elems=2, xy_size=8, p_random=0.5, cdf=(1 / 7, 4 / 7, 1.0))
    assert L.ogbx_play_plan(None, 4, 31, None, None, None, 0, None) == _lib.OGBX_EINVAL
    assert L.ogbx_play_plan(cfg, 4, 31, None, None, None, 0, None) == _lib.OGBX_EINVAL
    assert 'null' in _lib.last_error()
    assert L.ogbx_play_powder_reset(None, None, None, 0, None) == _lib.OGBX_EINVAL
    assert L.ogbx_play_sample_semantic(2, 8, 4, 0, 0, 0, None, None) == _lib.OGBX_EINVAL


@pytest.mark.parametrize('kw, match', [
    (dict(num_envs=0), 'num_envs'),
    (dict(num_rounds=0), 'num_rounds'),
    (dict(max_episode_steps=0), 'max_episode_steps'),
    (dict(chunk=0), 'chunk'),
    (dict(p_random_action=1.5), 'p_random_action'),
    (dict(p_random_action=-0.1), 'p_random_action'),
    (dict(num_envs=4, num_rounds=2, tape=np.zeros((1, 4, 10))), 'tape'),
])
def test_collect_powderworld_argument_checks(kw, match):
    from ogbench_amd.datagen import collect_powderworld

    with pytest.raises(ValueError, match=match):
        collect_powderworld(**kw)


def test_constructor_argument_checks():
    from ogbench_amd.powderworld import PowderworldEnv

    with pytest.raises(ValueError, match='auto_reset'):
        PowderworldEnv(mode='data_collection', auto_reset=True)
    with pytest.raises(ValueError, match='auto_reset'):
        PowderworldEnv(mode='data', auto_reset=True)
    with pytest.raises(AssertionError):
        PowderworldEnv(mode='collect')


def test_design_quotes_the_play_record():
    """Every measured number of DESIGN.md section 4.10 is the committed record's."""
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = json.load(open(os.path.join(root, 'profiles', 'play_collect.json')))
    doc = open(os.path.join(root, 'DESIGN.md')).read()
    assert 'profiles/play_collect.json' in doc
    assert f"{rec['plan']['median_us']:.0f} µs" in doc
    for name in ('easy', 'medium', 'hard'):
        e = rec['envs'][name]
        assert f"{e['collect_env_steps_per_s'] / 1e6:.1f} M" in doc
        assert f"{e['rollout_only_env_steps_per_s'] / 1e6:.1f} M" in doc
        assert e['collect_over_rollout'] > 1.0  # what the text says: collection is below rollout-only
    assert f"{rec['envs']['easy']['dataset_GB']:.1f} GB" in doc
    assert f"{rec['cpu_one_core']['plan_us_per_episode']:.0f} µs" in doc
    assert f"{rec['cpu_one_core']['easy_env_steps_per_s']:,}" in doc
