"""Env wrappers over the batched envs.

``FrameStack`` is the batched ``FrameStackWrapper`` of the reference
(impls/utils/env_utils.py:48-76): the stacked observation of every env is
composed on the device, one launch per step (include/ogbx_framestack.h).
"""

from __future__ import annotations

import numpy as np

from . import _framestack, _lib
from .spaces import Box


def _torch():
    import torch

    return torch


def stack_space(space, num_stack):
    """The Box of ``num_stack`` frames joined on the last axis: the same bounds
    and dtype, the last axis ``num_stack`` times as long (env_utils.py:57-59)."""
    low = np.concatenate([space.low] * num_stack, axis=-1)
    high = np.concatenate([space.high] * num_stack, axis=-1)
    return Box(low, high, low.shape, space.dtype)


class FrameStack:
    """``FrameStackWrapper(env, num_stack)`` for a ``MazeEnv`` (point or ant) or
    a ``PowderworldEnv``, in either mode.

    ``reset`` returns ``num_stack`` copies of the first frame, ``step`` (and
    ``wrap_step`` of ant handles) the last ``num_stack`` frames joined on the
    last axis, newest last; ``reset`` tiles ``info['goal']`` the same way.  With
    ``env.auto_reset`` an env that ends restarts its stack from the new
    episode's first observation, and ``info['final_observation']`` (where the
    env supplies one: the mazes) is the stack the reference's ``step`` returned
    before its ``reset``; only the rows of envs that ended this step are
    written.  Without ``auto_reset`` every env shifts, as in the reference, and
    the caller resets with ``mask=``.

    The returned tensors are views of buffers the wrapper owns: two stacks that
    alternate, so the observation returned by step t stays valid while step
    t + 1 is composed and is overwritten by step t + 2 (what
    ``add_step(observations, ..., next_observations)`` needs); ``reset``
    rewrites the current one in place; the goal stack and the final stack are
    one buffer each.  Clone what must live longer.

    Every other attribute is the wrapped env's.
    """

    def __init__(self, env, num_stack):
        k = int(num_stack)
        if k < 1:
            raise ValueError(f'num_stack must be >= 1, got {num_stack}')
        self.env = env
        self.num_stack = k
        self.single_observation_space = stack_space(env.single_observation_space, k)
        self.observation_space = stack_space(env.observation_space, k)
        self._stacks = None
        self._cur = 0
        self._shape = None
        self._final = None
        self._goal_stack = None
        self._goal_shape = None
        self._has_reset = False

    def __getattr__(self, name):  # reached only for what the wrapper itself lacks
        if name == 'env':
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    @property
    def auto_reset(self):
        return self.env.auto_reset

    @auto_reset.setter
    def auto_reset(self, value):
        self.env.auto_reset = value

    def _stacked_like(self, frame):
        torch = _torch()
        return torch.zeros(tuple(frame.shape[:-1]) + (frame.shape[-1] * self.num_stack,), dtype=frame.dtype,
                           device=frame.device)

    def _allocate(self, obs):
        self._stacks = [self._stacked_like(obs), self._stacked_like(obs)]
        self._shape = _framestack.shape_of(obs, self.num_stack)
        self._L = _framestack.bind()
        self._push = self._L.ogbx_framestack_push
        self._ptrs = [s.data_ptr() for s in self._stacks]
        self._obs_meta = (obs.shape, obs.dtype)
        torch = _torch()
        self._dev_idx = obs.device.index
        self._raw_stream = torch._C._cuda_getCurrentRawStream
        self._current_device = torch.cuda.current_device

    def _frame(self, obs):
        if (obs.shape, obs.dtype) != self._obs_meta:
            raise ValueError(f'the env returned an observation of shape {tuple(obs.shape)} / {obs.dtype}, the '
                             f'stack was built for {tuple(self._obs_meta[0])} / {self._obs_meta[1]}')
        return obs if obs.is_contiguous() else obs.contiguous()

    def reset(self, *, seed=None, options=None, mask=None):
        """``env.reset`` then the stack of every env (or those in ``mask``)
        becomes ``num_stack`` copies of its first frame.  Returns (stack, info),
        ``info['goal']`` tiled ``num_stack`` times on its last axis."""
        torch = _torch()
        obs, info = self.env.reset(seed=seed, options=options, mask=mask)
        if self._stacks is None:
            self._allocate(obs)
        obs = self._frame(obs)
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(obs.device, torch.uint8).contiguous()
        _framestack.fill(self._shape, obs, m, self._stacks[self._cur])
        if 'goal' in info:
            goal = info['goal'].contiguous()
            if self._goal_stack is None or self._goal_meta != (goal.shape, goal.dtype):
                self._goal_stack = self._stacked_like(goal)
                self._goal_shape = _framestack.shape_of(goal, self.num_stack)
                self._goal_meta = (goal.shape, goal.dtype)
            _framestack.fill(self._goal_shape, goal, m, self._goal_stack)
            info = dict(info, goal=self._goal_stack)
        self._has_reset = True
        return self._stacks[self._cur], info

    def _stacked(self, out):
        obs, reward, term, trunc, info = out
        obs = self._frame(obs)
        cur = self._cur
        auto = self.env.auto_reset
        final_obs = info.get('final_observation') if auto else None
        fin = None
        if final_obs is not None:
            final_obs = self._frame(final_obs)
            if self._final is None:
                self._final = self._stacked_like(obs)
            fin = self._final.data_ptr()
        if self._current_device() != self._dev_idx:
            with _torch().cuda.device(self._dev_idx):
                return self._stacked(out)
        st = self._push(self._shape, obs.data_ptr(), self._ptrs[cur], term.data_ptr() if auto else None,
                        trunc.data_ptr() if auto else None, None if fin is None else final_obs.data_ptr(),
                        self._ptrs[1 - cur], fin, self._raw_stream(self._dev_idx))
        if st:
            _lib.check(st, 'framestack_push')
        self._cur = 1 - cur
        if fin is not None:
            info = dict(info, final_observation=self._final)
        return self._stacks[1 - cur], reward, term, trunc, info

    def _check_reset(self):
        if not self._has_reset:
            raise RuntimeError('FrameStack.step before the first reset: there is no frame to stack onto')

    def step(self, action, **kw):
        """``env.step`` then one push.  Returns the env's tuple with the
        stacked observation (and the stacked ``info['final_observation']``)."""
        self._check_reset()
        return self._stacked(self.env.step(action, **kw))

    def wrap_step(self, qpos, qvel, **kw):
        """``env.wrap_step`` (ant handles) then one push."""
        self._check_reset()
        return self._stacked(self.env.wrap_step(qpos, qvel, **kw))
