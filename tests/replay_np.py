"""NumPy restatement of the batched replay-buffer semantics
(ogbench_amd.datasets.ReplayBuffer; reference impls/utils/datasets.py:86-146
applied N times in row order), shared by tests/test_replay_cpu.py and
tests/test_replay_gpu.py.  Casts are NumPy's own assignment casts."""

import numpy as np

SAC_KEYS = ('observations', 'actions', 'rewards', 'masks', 'next_observations')


def sequential_state(pointer, size, m, max_size):
    """(pointer, size) after m reference add_transition calls."""
    for _ in range(m):
        pointer = (pointer + 1) % max_size
        size = max(pointer, size)
    return pointer, size


def closed_state(pointer, size, m, max_size):
    """The same in closed form (what the insert kernel writes to its header):
    size' = max(size, the largest pointer value visited).  While size >=
    pointer or size == max_size - 1 -- every state the buffer reaches by
    itself -- this is max(size, min(pointer + m, max_size - 1)); the two other
    branches cover states a caller can set (size below the pointer)."""
    if m == 0:
        return pointer, size
    if pointer + m < max_size:
        top = pointer + m
    elif pointer < max_size - 1:
        top = max_size - 1
    else:  # from the last slot straight to 0: the pointers visited are 0 .. m - 1
        top = m - 1
    return (pointer + m) % max_size, max(size, top)


class ReplayNp:
    def __init__(self, columns, pointer=0, size=0):
        self.cols = {k: np.array(v) for k, v in columns.items()}
        self.max_size = max(len(v) for v in self.cols.values())
        self.pointer, self.size = pointer, size

    @classmethod
    def create(cls, example, max_size):
        cols = {}
        for k, v in example.items():
            v = np.array(v)
            cols[k] = np.zeros((max_size,) + v.shape, v.dtype)
        return cls(cols)

    @classmethod
    def create_from_initial_dataset(cls, init, max_size):
        cols = {}
        for k, v in init.items():
            cols[k] = np.zeros((max_size,) + v.shape[1:], v.dtype)
            cols[k][: len(v)] = v
        n = max(len(v) for v in init.values())
        return cls(cols, n, n)

    def add_transitions(self, batch, keep=None):
        n = len(next(iter(batch.values())))
        assert n <= self.max_size and set(batch) == set(self.cols)
        rows = np.arange(n) if keep is None else np.flatnonzero(np.asarray(keep))
        m = len(rows)
        if m:
            if self.pointer >= self.max_size:
                raise IndexError(self.pointer)
            slots = (self.pointer + np.arange(m)) % self.max_size
            for k, col in self.cols.items():
                with np.errstate(all='ignore'):
                    col[slots] = np.asarray(batch[k])[rows]
        self.pointer, self.size = closed_state(self.pointer, self.size, m, self.max_size)

    def add_step(self, observations, actions, rewards, terminated, next_observations, final_observation=None,
                 done=None, keep=None):
        nxt = np.asarray(next_observations)
        if final_observation is not None:
            d = np.asarray(done).astype(bool)
            nxt = np.where(d.reshape((-1,) + (1,) * (nxt.ndim - 1)), np.asarray(final_observation), nxt)
        # 1 - terminated in the column's dtype, after the cast
        masks = 1 - np.asarray(terminated).astype(self.cols['masks'].dtype)
        self.add_transitions(dict(observations=observations, actions=actions, rewards=rewards, masks=masks,
                                  next_observations=nxt), keep)

    def get_subset(self, idxs):
        idxs = np.asarray(idxs, np.int64)
        out = {k: v[idxs] for k, v in self.cols.items()}
        if 'next_observations' not in out:
            out['next_observations'] = self.cols['observations'][np.maximum(np.minimum(idxs + 1, self.size - 1), 0)]
        return out


def scenario(gold, name, part):
    """The arrays ``<name>_<part>_<key>`` of the fixture as a dict, in file order."""
    pre = f'{name}_{part}_'
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}
