"""GPU checks of powderworld play-data collection: the action-plan kernel
against the reference's recorded draws and actions, its Philox mode, the
data-collection mode of the envs and datagen.collect_powderworld, against
tests/golden/play_golden.npz (made by the reference's own code)."""

import os

import numpy as np
import pytest
import torch

import play_np

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'play_golden.npz')
SIZE = 8


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _plan(gpu, n, T, ne=2, **kw):
    from ogbench_amd import _play

    return _play.plan(n, T, size=SIZE, num_elems=ne, xy_size=SIZE, device=gpu, **kw)


@pytest.mark.parametrize('case', ['d', 'e', 'b', 'c'])
def test_plan_vs_tape(gpu, gold, case):
    E, T, ne, _ = (int(v) for v in gold[f'{case}_meta'])
    p = float(gold[f'{case}_p_random'])
    tape = gold[f'{case}_tape']
    if case in 'bc':  # T = 31 at N = 8: the two episodes four times over
        tape = np.concatenate([tape] * 4)
    assert tape.shape[0] == 8 and T in (1001, 31)
    ref = gold[f'{case}_actions'].reshape(E, T)
    out = _plan(gpu, 8, T, ne=ne, p_random_action=p, tape=tape, records=True)
    got = out['actions'].cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (T, 8)
    for e in range(8):
        assert np.array_equal(got[:, e], ref[e % E]), (case, e)
    assert np.array_equal(out['used'].cpu().numpy(), np.tile(gold[f'{case}_tape_len'], 8 // E))
    assert int(out['short_count'].item()) == 0
    term = out['terminals'].cpu().numpy()
    assert term.dtype == bool and term[-1] and not term[:-1].any()
    # the decision records are those of the restatement
    dec = out['decisions'].cpu().numpy()
    for e in range(E):
        n = int(gold[f'{case}_tape_len'][e])
        recs = play_np.plan_episode(gold[f'{case}_tape'][e, :n], T, SIZE, ne, p)[2]
        assert np.array_equal(dec[:, e], [play_np.pack_record(r) for r in recs])


def test_short_tape_raises_and_counts(gpu, gold):
    n = int(gold['d_tape_len'][0])
    tape = gold['d_tape'][:1, :n - 1]  # one value short
    with pytest.raises(ValueError, match='ran out') as ei:
        _plan(gpu, 1, 1001, p_random_action=0.5, tape=tape)
    assert ei.value.short_count == 1
    # a full tape of the same env does not
    assert int(_plan(gpu, 1, 1001, p_random_action=0.5, tape=gold['d_tape'][:1, :n])['short_count'].item()) == 0


def test_env_base_and_layout(gpu):
    kw = dict(p_random_action=0.5, seed=11, episode=3, records=True)
    p8 = _plan(gpu, 8, 1001, **kw)
    p3 = _plan(gpu, 3, 1001, env_base=5, **kw)
    p70 = _plan(gpu, 70, 1001, **kw)  # two waves
    for k in ('actions', 'decisions'):
        assert torch.equal(p3[k], p8[k][:, 5:8])
        assert torch.equal(p8[k], p70[k][:, :8])
    assert torch.equal(p3['used'], p8['used'][5:8]) and torch.equal(p8['used'], p70['used'][:8])


def test_plan_argument_checks(gpu):
    with pytest.raises(ValueError, match='T'):
        _plan(gpu, 4, 0)
    with pytest.raises(ValueError, match='p_random'):
        _plan(gpu, 4, 31, p_random_action=1.01)
    from ogbench_amd import _lib, _play

    L = _play.bind()
    cfg = _play.PlayConfig(size=8, num_elems=2, xy_size=8, p_random=0.5, cdf=(1 / 7, 4 / 7, 1.0))
    host = np.zeros((31, 4), np.int32)
    with torch.cuda.device(gpu):
        st = L.ogbx_play_plan(cfg, 4, 31, host.ctypes.data, None, None, 0, None)
    assert st == _lib.OGBX_EINVAL and 'device memory' in _lib.last_error()
    a = torch.zeros(31, 4, dtype=torch.int32, device=gpu)
    cfg.size = 1
    with torch.cuda.device(gpu):
        assert L.ogbx_play_plan(cfg, 4, 31, a.data_ptr(), None, None, 0, None) == _lib.OGBX_EINVAL


@pytest.fixture(scope='module')
def philox_plan(gpu):
    return _plan(gpu, 4096, 1001, ne=5, p_random_action=0.5, seed=7, records=True)


def test_philox_plan_is_valid_and_reproducible(gpu, philox_plan):
    a = philox_plan['actions']
    assert int(a.min()) >= 0
    assert int(a[0::3].max()) < 5 and int(a[1::3].max()) < 8 and int(a[2::3].max()) < 8
    again = _plan(gpu, 4096, 1001, ne=5, p_random_action=0.5, seed=7, records=True)
    assert torch.equal(a, again['actions']) and torch.equal(philox_plan['used'], again['used'])
    other = _plan(gpu, 4096, 1001, ne=5, p_random_action=0.5, seed=7, episode=1)
    assert not torch.equal(a, other['actions'])
    assert not torch.equal(a[:, :2048], a[:, 2048:])  # envs differ


def test_philox_plan_statistics(philox_plan):
    dec = philox_plan['decisions'].cpu().numpy().astype(np.int64)
    n = dec.size
    frac = (dec & 1).mean()
    assert abs(frac - 0.5) <= 5 * np.sqrt(0.5 * 0.5 / n), (frac, n)
    kinds = (dec[(dec >> 3) & 1 == 1] >> 1) & 3  # the behaviour choices: decisions with a fresh behaviour
    m = kinds.size
    assert m > 4096
    for k, pk in enumerate((1 / 7, 3 / 7, 3 / 7)):
        fk = (kinds == k).mean()
        assert abs(fk - pk) <= 5 * np.sqrt(pk * (1 - pk) / m), (k, fk, m)


def test_sample_semantic_action(gpu):
    import ogbench_amd

    env = ogbench_amd.make('powderworld-hard-v0', num_envs=4096, device=gpu, mode='data_collection', seed=3)
    env.reset()
    s1, s2 = env.sample_semantic_action(), env.sample_semantic_action()
    assert s1.dtype == torch.int32 and tuple(s1.shape) == (4096, 3)
    assert int(s1.min()) >= 0 and int(s1[:, 0].max()) == 7 and int(s1[:, 1:].max()) == 7
    assert not torch.equal(s1, s2)
    a = env.sample_action()
    assert tuple(a.shape) == (4096,) and int(a.max()) == 7  # stage 0: an element
    env.close()


def _empty_world_obs():
    img = np.zeros((32, 32, 6), np.uint8)
    img[..., :3] = (236, 240, 241)
    for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
        img[sl + (slice(0, 3),)] = (108, 122, 137)
    return img


def test_collect_easy_equals_the_reference(gpu, gold):
    from ogbench_amd.datagen import collect_powderworld

    E, T = 2, 61
    data = collect_powderworld('powderworld-easy-v0', num_envs=E, num_rounds=1, max_episode_steps=T,
                               p_random_action=0.5, device=gpu, chunk=16, tape=gold['a_tape'][None])
    assert data['observations'].dtype == torch.uint8 and data['actions'].dtype == torch.int32
    assert data['terminals'].dtype == torch.bool
    assert np.array_equal(data['actions'].cpu().numpy(), gold['a_actions'])
    assert np.array_equal(data['terminals'].cpu().numpy(), gold['a_terminals'])
    got, ref = data['observations'].cpu().numpy(), gold['a_obs']
    assert got.shape == ref.shape
    bad = np.nonzero((got != ref).reshape(E * T, -1).any(1))[0]
    assert bad.size == 0, f'rows {bad[:8]} differ'
    assert np.array_equal(ref[0], _empty_world_obs())


@pytest.mark.parametrize('case, name', [('b', 'powderworld-medium-v0'), ('c', 'powderworld-hard-v0')])
def test_data_mode_full_equals_the_reference(gpu, gold, case, name):
    import ogbench_amd

    E, T, ne, H = (int(v) for v in gold[f'{case}_meta'])
    env = ogbench_amd.make(name, num_envs=E, device=gpu, mode='data_collection', max_episode_steps=T)
    ob, info = env.reset(seed=0)
    assert info == {}
    ref = gold[f'{case}_obs'].reshape(E, T, H, H, 6)
    assert np.array_equal(ob.cpu().numpy(), ref[:, 0])
    acts = gold[f'{case}_actions'].reshape(E, T).T.copy()
    rand = np.zeros((T, E, 3, H, H), np.float32)
    rand[2::3] = gold[f'{case}_rand'].transpose(1, 0, 2, 3, 4)  # forward q is the one of step 3q + 2
    out = env.rollout(acts, rand=rand)
    assert 'success' not in out
    got = out['obs'].cpu().numpy()
    for t in range(T - 1):
        assert np.array_equal(got[t], ref[:, t + 1]), (case, t)
    assert float(out['reward'].abs().max()) == 0.0 and int(out['terminated'].max()) == 0
    trunc = out['truncated'].cpu().numpy()
    assert trunc[-1].all() and not trunc[:-1].any()
    env.close()


def test_data_mode_step_and_masked_reset(gpu):
    import ogbench_amd

    env = ogbench_amd.make('powderworld-easy-v0', num_envs=3, device=gpu, mode='data', max_episode_steps=4)
    assert env._mode == 'data_collection'
    ob, info = env.reset(seed=1)
    blank = ob.clone()
    assert info == {} and np.array_equal(blank[0].cpu().numpy(), _empty_world_obs())
    for t, a in enumerate((1, 2, 3, 0)):
        ob, rew, term, trunc, info = env.step([a] * 3)
        assert info == {} and float(rew.max()) == 0.0 and not bool(term.any())
        assert bool(trunc.all()) == (t == 3)
    assert not torch.equal(ob, blank)  # the painted stone is there
    painted = ob.clone()
    ob, _ = env.reset(mask=[1, 0, 0])
    assert torch.equal(ob[0], blank[0]) and torch.equal(ob[1:], painted[1:])
    assert env._scalar_view('elapsed').tolist() == [0, 4, 4]
    with pytest.raises(ValueError, match='no options'):
        env.reset(options=dict(task_id=1))
    env.close()


def test_collect_without_a_tape(gpu):
    from ogbench_amd.datagen import collect_powderworld

    N, T, R = 4, 31, 2
    data = collect_powderworld('powderworld-medium-v0', num_envs=N, num_rounds=R, max_episode_steps=T, seed=5,
                               device=gpu, chunk=7)
    obs, act, term = data['observations'], data['actions'], data['terminals']
    assert tuple(obs.shape) == (R * N * T, 32, 32, 6) and obs.dtype == torch.uint8
    assert tuple(act.shape) == (R * N * T,) and act.dtype == torch.int32
    assert tuple(term.shape) == (R * N * T,) and term.dtype == torch.bool
    want = (torch.arange(R * N * T, device=term.device) % T) == T - 1
    assert torch.equal(term, want)
    rows0 = obs.reshape(R * N, T, 32, 32, 6)[:, 0].cpu().numpy()
    assert all(np.array_equal(r, _empty_world_obs()) for r in rows0)
    a = act.reshape(R, N, T)
    assert not torch.equal(a[0], a[1])  # rounds differ
    assert int(a[..., 0::3].max()) < 5 and int(a.max()) < 8 and int(a.min()) >= 0
    o = obs.reshape(R, N * T, -1)
    assert not torch.equal(o[0], o[1])
