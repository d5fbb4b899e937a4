"""CPU checks of the frame-stack feature's host side: the NumPy restatement
(tests/framestack_np.py) against the reference's FrameStackWrapper
(tests/golden/framestack_golden.npz, written by make_golden_framestack.py), the
exports of include/ogbx_framestack.h, every OGBX_EINVAL of its entry points
(all raised before a device is touched), FrameStack's argument and space
arithmetic, and env_utils.make_env_and_datasets' pass-through."""

import ctypes
import os
import re

import numpy as np
import pytest

import framestack_np as fnp
from ogbench_amd import _framestack, _lib, env_utils, wrappers
from ogbench_amd.spaces import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('vec_a', 'vec_b', 'img_a', 'img_b')
KS = (1, 2, 3, 4)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'framestack_golden.npz')))


def test_golden_histories_are_the_designed_ones(golden):
    for frame in ('vec', 'img'):
        a = golden[f'{frame}_a_terminated'] | golden[f'{frame}_a_truncated']
        b = golden[f'{frame}_b_terminated'] | golden[f'{frame}_b_truncated']
        assert a.shape == (13, 4)
        assert a[0, 0] and a[4, 1] and a[5, 1] and not a[:, 2].any() and not a.all(1).any()
        assert b.all(1).sum() == 1 and np.array_equal(b[np.arange(13) != 7], a[np.arange(13) != 7])
        kinds = {(int(t), int(u)) for t, u in zip(golden[f'{frame}_b_terminated'].ravel(),
                                                  golden[f'{frame}_b_truncated'].ravel())}
        assert kinds == {(0, 0), (1, 0), (0, 1), (1, 1)}
    assert golden['vec_a_frames'].shape == (13, 4, 2) and golden['vec_a_frames'].dtype == np.float64
    assert golden['img_a_frames'].shape == (13, 4, 3, 5, 6) and golden['img_a_frames'].dtype == np.uint8


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('k', KS)
def test_restatement_reproduces_the_reference_wrapper(golden, case, k):
    g = lambda name: golden[f'{case}_{name}']  # noqa: E731
    gk = lambda name: golden[f'{case}_k{k}_{name}']  # noqa: E731
    frames, resets, goals = g('frames'), g('reset_frames'), g('goals')
    term, trunc = g('terminated'), g('truncated')
    done = (term | trunc).astype(bool)
    # reset, and the goal tiling
    stack = fnp.fill(resets[0], k)
    assert np.array_equal(stack, gk('stack0'))
    assert np.array_equal(fnp.fill(goals[0], k), gk('goal0'))
    manual = stack.copy()
    final = np.zeros_like(stack)
    for t in range(frames.shape[0]):
        # same-step auto-reset: obs is the reset frame on a done step, final_obs the step's own
        obs = np.where(done[t].reshape((-1,) + (1,) * (frames.ndim - 2)), resets[t + 1], frames[t])
        stack, final = fnp.push(obs, stack, k, term[t], trunc[t], frames[t], final)
        assert np.array_equal(stack, gk('stacks')[t]), t
        assert np.array_equal(final[done[t]], gk('final')[t][done[t]]), t
        # manual reset: every env shifts, then fill(mask) restarts the done ones
        manual, none = fnp.push(frames[t], manual, k)
        assert none is None
        assert np.array_equal(manual[done[t]], gk('final')[t][done[t]]), t
        manual = fnp.fill(resets[t + 1], k, done[t], manual)
        assert np.array_equal(manual, gk('stacks')[t]), t
        tiles = fnp.fill(goals[t + 1], k, done[t], np.zeros_like(gk('goal_tiles')[t]))
        assert np.array_equal(tiles, gk('goal_tiles')[t]), t
    # final rows of envs that were never done keep what they held
    assert not final[~done.any(0)].any()


def test_library_exports_the_framestack_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ogbx_framestack.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(ogbx_[a-z0-9_]+)\s*\(', text)))
    assert declared == ['ogbx_framestack_abi_version', 'ogbx_framestack_fill', 'ogbx_framestack_push']
    L = _framestack.bind()
    assert [s for s in declared if not hasattr(L, s)] == []
    assert L.ogbx_framestack_abi_version() == _framestack.FRAMESTACK_ABI_VERSION == 1
    assert int(re.search(r'#define\s+OGBX_FRAMESTACK_ABI_VERSION\s+(\d+)', text).group(1)) == 1
    assert L.ogbx_abi_version() == 5  # ogbx.h's own version is untouched by the extension
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert [s for s in declared if s not in doc] == []
    assert 'ogbx_framestack.h' in open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert ctypes.sizeof(_framestack.FrameStackShape) == 32 and _framestack.FrameStackShape.num_stack.offset == 24


# never dereferenced: every case below returns before any device work
OBS, PREV, NEXT, FINAL, FOBS, TERM, TRUNC = (0x10000 * (i + 1) for i in range(7))


def _shape(n=4, pixels=5, elem_bytes=6, num_stack=3):
    return _framestack.FrameStackShape(n=n, pixels=pixels, elem_bytes=elem_bytes, num_stack=num_stack, pad=0)


def _push(shape=None, obs=OBS, prev=PREV, term=TERM, trunc=TRUNC, fobs=FOBS, nxt=NEXT, final=FINAL):
    L = _framestack.bind()
    return L.ogbx_framestack_push(_shape() if shape is None else shape, obs, prev, term, trunc, fobs, nxt, final, None)


def _fill(shape=None, obs=OBS, mask=TERM, stack=NEXT):
    L = _framestack.bind()
    return L.ogbx_framestack_fill(_shape() if shape is None else shape, obs, mask, stack, None)


BIG = 1 << 62
PUSH_EINVAL = {
    'null shape': (lambda: _framestack.bind().ogbx_framestack_push(None, OBS, PREV, TERM, TRUNC, FOBS, NEXT, FINAL,
                                                                   None), 'null shape'),
    'null obs': (lambda: _push(obs=None), 'null'),
    'null prev': (lambda: _push(prev=None), 'null'),
    'null next': (lambda: _push(nxt=None), 'null'),
    'n < 0': (lambda: _push(_shape(n=-1)), 'n must be'),
    'pixels < 1': (lambda: _push(_shape(pixels=0)), 'pixels'),
    'elem_bytes < 1': (lambda: _push(_shape(elem_bytes=0)), 'elem_bytes'),
    'num_stack < 1': (lambda: _push(_shape(num_stack=0)), 'num_stack'),
    'row overflow': (lambda: _push(_shape(pixels=BIG, elem_bytes=BIG)), 'int64'),
    'total overflow': (lambda: _push(_shape(n=BIG, pixels=1, elem_bytes=8, num_stack=2)), 'int64'),
    'final_stack without final_obs': (lambda: _push(fobs=None), 'final_obs'),
    'final_stack without masks': (lambda: _push(term=None, trunc=None), 'mask'),
    'unaligned next': (lambda: _push(nxt=NEXT + 8), '16-byte'),
    'unaligned prev': (lambda: _push(prev=PREV + 4), '16-byte'),
    'unaligned final_stack': (lambda: _push(final=FINAL + 2), '16-byte'),
    'next is prev': (lambda: _push(nxt=PREV), 'next overlaps prev'),
    'next meets the end of prev': (lambda: _push(nxt=PREV + 352), 'next overlaps prev'),  # 4 * 5 * 18 = 360 bytes
    'next meets obs': (lambda: _push(obs=NEXT + 350), 'next overlaps obs'),
    'next meets truncated': (lambda: _push(trunc=NEXT + 359), 'next overlaps truncated'),
    'final_stack is next': (lambda: _push(final=NEXT), 'overlaps'),
    'final_stack meets final_obs': (lambda: _push(fobs=FINAL + 16), 'final_stack overlaps final_obs'),
    'final_stack meets terminated': (lambda: _push(term=FINAL), 'final_stack overlaps terminated'),
}
FILL_EINVAL = {
    'null shape': (lambda: _framestack.bind().ogbx_framestack_fill(None, OBS, None, NEXT, None), 'null shape'),
    'null obs': (lambda: _fill(obs=None), 'null'),
    'null stack': (lambda: _fill(stack=None), 'null'),
    'n < 0': (lambda: _fill(_shape(n=-2)), 'n must be'),
    'pixels < 1': (lambda: _fill(_shape(pixels=-1)), 'pixels'),
    'elem_bytes < 1': (lambda: _fill(_shape(elem_bytes=0)), 'elem_bytes'),
    'num_stack < 1': (lambda: _fill(_shape(num_stack=-3)), 'num_stack'),
    'overflow': (lambda: _fill(_shape(n=1 << 40, pixels=1 << 20, elem_bytes=8, num_stack=2)), 'int64'),
    'unaligned stack': (lambda: _fill(stack=NEXT + 1), '16-byte'),
    'stack meets obs': (lambda: _fill(obs=NEXT + 359), 'stack overlaps obs'),
    'stack meets mask': (lambda: _fill(mask=NEXT + 16), 'stack overlaps mask'),
}


@pytest.mark.parametrize('name', sorted(PUSH_EINVAL))
def test_push_refuses_before_any_device(name):
    call, match = PUSH_EINVAL[name]
    assert call() == _lib.OGBX_EINVAL
    msg = _lib.last_error()
    assert msg.startswith('ogbx_framestack_push: ') and match in msg, msg


@pytest.mark.parametrize('name', sorted(FILL_EINVAL))
def test_fill_refuses_before_any_device(name):
    call, match = FILL_EINVAL[name]
    assert call() == _lib.OGBX_EINVAL
    msg = _lib.last_error()
    assert msg.startswith('ogbx_framestack_fill: ') and match in msg, msg


def test_adjacent_ranges_and_zero_envs_are_accepted_without_a_device():
    # n == 0: nothing to launch, nothing to check against a device; ranges are empty
    assert _push(_shape(n=0)) == _lib.OGBX_OK
    assert _push(_shape(n=0), nxt=PREV, final=None, fobs=None) == _lib.OGBX_OK
    assert _fill(_shape(n=0)) == _lib.OGBX_OK
    assert _fill(_shape(n=0), mask=None) == _lib.OGBX_OK


class _Env:
    """What FrameStack reads of an env before its first reset."""

    auto_reset = True
    num_envs = 7
    marker = 'delegated'

    def __init__(self, single, batched):
        self.single_observation_space, self.observation_space = single, batched

    @property
    def unwrapped(self):
        return self


def test_framestack_refuses_num_stack_below_one():
    env = _Env(Box(0, 255, (3, 5, 6), np.uint8), Box(0, 255, (7, 3, 5, 6), np.uint8))
    for k in (0, -1):
        with pytest.raises(ValueError, match='num_stack'):
            wrappers.FrameStack(env, k)


@pytest.mark.parametrize('k', KS)
def test_framestack_spaces_and_delegation(golden, k):
    env = _Env(Box(0, 255, (3, 5, 6), np.uint8), Box(0, 255, (7, 3, 5, 6), np.uint8))
    w = wrappers.FrameStack(env, k)
    assert w.num_stack == k and w.unwrapped is env and w.env is env
    assert w.single_observation_space.shape == tuple(golden[f'img_a_k{k}_space_shape']) == (3, 5, 6 * k)
    assert w.single_observation_space.dtype == np.uint8
    assert np.array_equal(w.single_observation_space.low, golden[f'img_a_k{k}_space_low'])
    assert np.array_equal(w.single_observation_space.high, golden[f'img_a_k{k}_space_high'])
    assert w.observation_space.shape == (7, 3, 5, 6 * k)
    assert w.observation_space.low.min() == 0 and w.observation_space.high.max() == 255
    venv = _Env(Box(-np.inf, np.inf, (2,), np.float64), Box(-np.inf, np.inf, (7, 2), np.float64))
    v = wrappers.FrameStack(venv, k)
    assert v.single_observation_space.shape == tuple(golden[f'vec_a_k{k}_space_shape']) == (2 * k,)
    assert v.single_observation_space.dtype == np.float64
    assert np.array_equal(v.single_observation_space.low, golden[f'vec_a_k{k}_space_low'])
    assert np.array_equal(v.single_observation_space.high, golden[f'vec_a_k{k}_space_high'])
    assert v.observation_space.shape == (7, 2 * k)
    # everything else is the env's
    assert w.auto_reset is True and w.num_envs == 7 and w.marker == 'delegated'
    w.auto_reset = False
    assert env.auto_reset is False
    with pytest.raises(AttributeError):
        w.no_such_attribute
    with pytest.raises(RuntimeError, match='before the first reset'):
        w.step(None)
    with pytest.raises(RuntimeError, match='before the first reset'):
        w.wrap_step(None, None)


def test_package_exports_framestack():
    import ogbench_amd

    assert ogbench_amd.FrameStack is wrappers.FrameStack and 'FrameStack' in ogbench_amd.__all__


@pytest.mark.parametrize('frame_stack', (None, 3))
def test_make_env_and_datasets_passes_its_arguments_through(monkeypatch, frame_stack):
    calls = []

    class Env(_Env):
        resets = 0

        def reset(self, **kw):
            assert not kw
            Env.resets += 1
            return None, {}

    env = Env(Box(0, 255, (3, 5, 6), np.uint8), Box(0, 255, (2, 3, 5, 6), np.uint8))

    def fake(dataset_name, **kw):
        calls.append((dataset_name, kw))
        return env, {'observations': 'train'}, {'observations': 'val'}

    monkeypatch.setattr(env_utils.utils, 'make_env_and_datasets', fake)
    # the wrapper's own reset needs a device; here it is only counted
    monkeypatch.setattr(wrappers.FrameStack, 'reset', lambda self, **kw: self.env.reset(**kw))
    got, train, val = env_utils.make_env_and_datasets('powderworld-easy-play-v0', frame_stack=frame_stack,
                                                      dataset_path='/data/x.npz', num_envs=2, device='cuda:0')
    assert calls == [('powderworld-easy-play-v0', dict(dataset_path='/data/x.npz', compact_dataset=True, num_envs=2,
                                                       device='cuda:0'))]
    assert train == {'observations': 'train'} and val == {'observations': 'val'}
    assert Env.resets == 1
    if frame_stack is None:
        assert got is env
    else:
        assert isinstance(got, wrappers.FrameStack) and got.env is env and got.num_stack == 3
        assert got.single_observation_space.shape == (3, 5, 18)
