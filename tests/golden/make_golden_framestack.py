"""Golden fixture for frame-stacked envs, from the reference's own
FrameStackWrapper (impls/utils/env_utils.py:48-76).

gymnasium is not a dependency here, so env_utils.py is loaded over in-process
stand-ins: a minimal ``gymnasium.Wrapper``, ``gymnasium.spaces.Box`` and stubs
for ``ogbench`` and ``utils.datasets`` (which FrameStackWrapper does not use).
The wrapper is driven over a scripted single env, one wrapper per env lane,
with ``reset`` after a done step as same-step auto-reset does.  Saves arrays
only (tests/golden/framestack_golden.npz).

4 lanes, 13 steps, k in {1, 2, 3, 4}, frames ``vec`` (2,) float64 and ``img``
(3, 5, 6) uint8, each under two designed done histories (no lane can both be
"never done" and take part in a step where every lane is done):
  a  lane 0 done on its first step (and step 8), lane 1 done on the consecutive
     steps 4 and 5, lane 2 never done, lane 3 done on the last step
  b  history a plus step 7, on which every lane is done
A done step is terminated, truncated or both, in turn.  Every byte encodes
(lane, step, pixel, channel); reset frames and goals use their own codes.

Per case <c> = <frame>_<history>:
  <c>_frames        [T, L, ...]     what env.step returned (final_obs on a done step)
  <c>_reset_frames  [T + 1, L, ...] [0]: the first reset; [t + 1]: the reset after a done step t (else zeros)
  <c>_goals         [T + 1, L, ...] info['goal'] of those resets
  <c>_terminated, <c>_truncated  [T, L] u8
and per k:
  <c>_k<k>_stack0   [L, ...k]       the first reset's stack
  <c>_k<k>_goal0    [L, ...k]       its tiled goal
  <c>_k<k>_stacks   [T, L, ...k]    the observation after step t: the wrapper's step output, or on a done
                                    step the stack its reset returned
  <c>_k<k>_final    [T, L, ...k]    the wrapper's step output on a done step (else zeros)
  <c>_k<k>_goal_tiles [T, L, ...k]  the tiled goal of the reset after a done step (else zeros)
  <c>_k<k>_space_shape, _space_low, _space_high  the wrapper's observation_space
"""

import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_gc as gg  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
L, T = 4, 13
KS = (1, 2, 3, 4)
FRAMES = {'vec': ((2,), np.float64), 'img': ((3, 5, 6), np.uint8)}


class Box:
    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        shape = np.shape(low) if shape is None else tuple(shape)
        self.low = np.broadcast_to(np.asarray(low, self.dtype), shape).copy()
        self.high = np.broadcast_to(np.asarray(high, self.dtype), shape).copy()
        self.shape = tuple(shape)


class Wrapper:
    """What FrameStackWrapper uses of gymnasium.Wrapper: ``env`` and an
    ``observation_space`` that falls through to the env's until it is set."""

    def __init__(self, env):
        self.env = env
        self._observation_space = None

    @property
    def observation_space(self):
        return self.env.observation_space if self._observation_space is None else self._observation_space

    @observation_space.setter
    def observation_space(self, space):
        self._observation_space = space


def reference_env_utils():
    gym = types.ModuleType('gymnasium')
    spaces = types.ModuleType('gymnasium.spaces')
    gym.Wrapper, gym.spaces, spaces.Box = Wrapper, spaces, Box
    ogb = types.ModuleType('ogbench')
    utils = types.ModuleType('utils')
    utils.__path__ = []
    uds = types.ModuleType('utils.datasets')
    uds.Dataset = type('Dataset', (), {})
    sys.modules.update({'gymnasium': gym, 'gymnasium.spaces': spaces, 'ogbench': ogb, 'utils': utils,
                        'utils.datasets': uds})
    return gg._load('ref_env_utils', os.path.join(gg.REF, 'impls/utils/env_utils.py'))


def code(kind, lane, step, shape, dtype):
    """A frame whose every element encodes (kind, lane, step, pixel, channel)."""
    idx = np.indices(shape)
    chan = idx[-1]
    pix = np.zeros(shape, np.int64)
    for ax in range(len(shape) - 1):
        pix = pix * shape[ax] + idx[ax]
    if np.dtype(dtype) == np.uint8:
        return ((kind * 97 + lane * 61 + step * 17 + pix * 7 + chan * 3 + 1) % 251).astype(np.uint8)
    return (kind * 1e6 + lane * 1e4 + step * 1e2 + pix * 10 + chan + 0.5).astype(dtype) * (-1.0 if kind else 1.0)


def histories():
    a = np.zeros((T, L), np.uint8)
    a[0, 0] = a[8, 0] = 1
    a[4, 1] = a[5, 1] = 1
    a[T - 1, 3] = 1
    b = a.copy()
    b[7, :] = 1
    out = {}
    for name, done in (('a', a), ('b', b)):
        term, trunc = np.zeros_like(done), np.zeros_like(done)
        for i, (t, lane) in enumerate(np.argwhere(done)):  # terminated, truncated, both, in turn
            term[t, lane] = i % 3 != 1
            trunc[t, lane] = i % 3 != 0
        assert np.array_equal(term | trunc, done)
        out[name] = (term, trunc)
    assert a[:, 2].sum() == 0 and b[7].all() and a[0, 0] and a[4, 1] and a[5, 1]
    return out


class ScriptedEnv:
    """One lane: replays its frames, done flags, reset frames and goals."""

    def __init__(self, frames, term, trunc, reset_frames, goals, space):
        self.frames, self.term, self.trunc = frames, term, trunc
        self.reset_frames, self.goals = reset_frames, goals
        self.observation_space = space
        self.t = 0

    def reset(self, **kwargs):
        i = self.t  # reset number 0 comes before step 0, number t + 1 after step t
        return self.reset_frames[i].copy(), {'goal': self.goals[i].copy()}

    def step(self, action):
        t = self.t
        self.t += 1
        return self.frames[t].copy(), 0.0, bool(self.term[t]), bool(self.trunc[t]), {}


def main():
    ref = reference_env_utils()
    out = {}
    for fname, (shape, dtype) in FRAMES.items():
        info = np.iinfo(dtype) if np.dtype(dtype) == np.uint8 else None
        low, high = (info.min, info.max) if info else (-np.inf, np.inf)
        for hname, (term, trunc) in histories().items():
            c = f'{fname}_{hname}'
            done = (term | trunc).astype(bool)
            frames = np.stack([np.stack([code(0, lane, t, shape, dtype) for lane in range(L)]) for t in range(T)])
            resets = np.zeros((T + 1, L) + shape, dtype)
            goals = np.zeros((T + 1, L) + shape, dtype)
            for lane in range(L):
                for i in range(T + 1):
                    if i == 0 or done[i - 1, lane]:
                        resets[i, lane] = code(1, lane, i, shape, dtype)
                        goals[i, lane] = code(2, lane, i, shape, dtype)
            out[f'{c}_frames'], out[f'{c}_reset_frames'], out[f'{c}_goals'] = frames, resets, goals
            out[f'{c}_terminated'], out[f'{c}_truncated'] = term, trunc
            for k in KS:
                kshape = shape[:-1] + (shape[-1] * k,)
                stack0, goal0 = np.zeros((L,) + kshape, dtype), np.zeros((L,) + kshape, dtype)
                stacks, final, tiles = (np.zeros((T, L) + kshape, dtype) for _ in range(3))
                for lane in range(L):
                    env = ScriptedEnv(frames[:, lane], term[:, lane], trunc[:, lane], resets[:, lane],
                                      goals[:, lane], Box(low, high, shape, dtype))
                    w = ref.FrameStackWrapper(env, k)
                    ob, inf = w.reset()
                    stack0[lane], goal0[lane] = ob, inf['goal']
                    for t in range(T):
                        ob, _, te, tr, _ = w.step(None)
                        if te or tr:
                            final[t, lane] = ob
                            ob, inf = w.reset()
                            tiles[t, lane] = inf['goal']
                        stacks[t, lane] = ob
                    sp = w.observation_space
                    assert sp.dtype == np.dtype(dtype)
                out[f'{c}_k{k}_stack0'], out[f'{c}_k{k}_goal0'] = stack0, goal0
                out[f'{c}_k{k}_stacks'], out[f'{c}_k{k}_final'], out[f'{c}_k{k}_goal_tiles'] = stacks, final, tiles
                out[f'{c}_k{k}_space_shape'] = np.array(sp.shape, np.int64)
                out[f'{c}_k{k}_space_low'], out[f'{c}_k{k}_space_high'] = sp.low, sp.high
    path = os.path.join(OUT, 'framestack_golden.npz')
    np.savez_compressed(path, **out)
    print('framestack golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
