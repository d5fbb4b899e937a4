"""NumPy restatement of ogbx_framestack_fill / ogbx_framestack_push
(include/ogbx_framestack.h): per env a ring (deque) of its last k frames, the
stack being their concatenation on the last axis, as FrameStackWrapper
(impls/utils/env_utils.py:48-76) keeps it.  No byte arithmetic: frames are
split off and joined as arrays.
"""

import collections

import numpy as np


def _ring(stack_e, k):
    """One env's stack [..., k*C] as a deque of its k frames [..., C]."""
    return collections.deque(np.split(stack_e, k, axis=-1), maxlen=k)


def _join(ring):
    return np.concatenate(list(ring), axis=-1)


def fill(obs, k, mask=None, stack=None):
    """All k slots of stack[e] become obs[e], for every env or those with
    mask[e] != 0; other rows keep what ``stack`` holds.  Returns a new array."""
    obs = np.asarray(obs)
    n = obs.shape[0]
    shape = obs.shape[:-1] + (obs.shape[-1] * k,)
    out = np.zeros(shape, obs.dtype) if stack is None else np.array(stack, copy=True)
    assert out.shape == shape and out.dtype == obs.dtype
    for e in range(n):
        if mask is None or mask[e]:
            out[e] = _join(collections.deque([obs[e]] * k, maxlen=k))
    return out


def push(obs, prev, k, terminated=None, truncated=None, final_obs=None, final_stack=None):
    """One step.  Returns (next, final_stack): final_stack is None unless one
    was passed in, and then only its done rows are replaced."""
    obs, prev = np.asarray(obs), np.asarray(prev)
    n = obs.shape[0]
    done = np.zeros(n, bool)
    for m in (terminated, truncated):
        if m is not None:
            done |= np.asarray(m).astype(bool)
    nxt = np.empty_like(prev)
    fin = None if final_stack is None else np.array(final_stack, copy=True)
    for e in range(n):
        ring = _ring(prev[e], k)
        if done[e]:
            if fin is not None:
                last = _ring(prev[e], k)
                last.append(final_obs[e])
                fin[e] = _join(last)
            ring = collections.deque([obs[e]] * k, maxlen=k)
        else:
            ring.append(obs[e])
        nxt[e] = _join(ring)
    return nxt, fin
