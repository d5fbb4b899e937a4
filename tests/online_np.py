"""tests/online_np.py -- TEST INFRASTRUCTURE ONLY.

NumPy restatement of the episode ring of include/ogbx_online.h
(``ogbench_amd.datasets.GCReplayBuffer``): the time-major ring, the
``ep_seq`` / ``cur_seq`` / ``ep_end`` tables kept at O(1) per inserted row, the
unrolling of the live rows into the snapshot dataset, and the flat-to-physical
row map.  ``Brute`` is the model it is checked against: each env's full history
as Python lists, the snapshot built from those with no table at all.

The sample itself is ``oracle/gcdataset_np.sample`` over the snapshot (the
restatement of the reference's ``GCDataset.sample``).
"""

import numpy as np

from oracle import gcdataset_np as gco


# the configs of tests/golden/online_golden.npz: geometric / uniform trajectory goals x gc_negative on / off
def _cfg(geom, negative):
    return dict(discount=0.7, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3,
                value_geom_sample=geom, actor_p_curgoal=0.1, actor_p_trajgoal=0.6, actor_p_randomgoal=0.3,
                actor_geom_sample=geom, gc_negative=negative, p_aug=None, frame_stack=None)


GOLDEN_CONFIGS = {'geom_neg': _cfg(True, True), 'geom_pos': _cfg(True, False), 'unif_neg': _cfg(False, True),
                  'unif_pos': _cfg(False, False)}


def _np_dtype(example):
    return np.array(example).dtype


class OnlineNp:
    def __init__(self, example, num_envs, horizon):
        self.N, self.T, self.S = int(num_envs), int(horizon), 0
        self.cols = {k: np.zeros((self.T * self.N,) + np.array(v).shape, _np_dtype(v)) for k, v in example.items()}
        self.ep_seq = np.zeros((self.T, self.N), np.int32)
        self.cur_seq = np.zeros(self.N, np.int32)
        self.ep_end = np.zeros((self.T, self.N), np.int64)

    @property
    def L(self):
        return min(self.S, self.T)

    def clear(self):
        self.S = 0
        self.cur_seq[:] = 0

    def add(self, batch, done):
        """One row per env at step S; returns the physical rows written."""
        N, T, S = self.N, self.T, self.S
        assert set(batch) == set(self.cols)
        done = np.asarray(done).astype(bool)
        assert done.shape == (N,)
        slot = S % T
        rows = slot * N + np.arange(N)
        for k, col in self.cols.items():
            v = np.asarray(batch[k])
            assert v.shape == (N,) + col.shape[1:], k
            col[rows] = v  # NumPy's assignment cast
        self.ep_seq[slot] = self.cur_seq
        e = np.flatnonzero(done)
        self.ep_end[self.cur_seq[e] % T, e] = S
        self.cur_seq[e] += 1
        self.S = S + 1
        return rows

    def add_step(self, observations, actions, terminated, truncated, next_observations, final_observation=None):
        done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
        nxt = np.asarray(next_observations)
        if final_observation is not None:
            nxt = np.where(done.reshape((-1,) + (1,) * (nxt.ndim - 1)), np.asarray(final_observation), nxt)
        return self.add(dict(observations=observations, actions=actions, next_observations=nxt,
                             terminals=done.astype(np.float32)), done)

    # ------------------------------------------------------------- the unrolling
    def split(self, flat):
        flat = np.asarray(flat, np.int64)
        return flat // self.L, flat % self.L

    def phys(self, flat):
        """Physical row of every flat snapshot index."""
        e, k = self.split(flat)
        return ((self.S - self.L + k) % self.T) * self.N + e

    def end_steps(self):
        """[N, L]: the logical step at which each live row's episode ends, read
        from the tables as the kernel reads them."""
        N, T, S, L = self.N, self.T, self.S, self.L
        steps = np.arange(S - L, S)
        seq = self.ep_seq[steps % T].T  # [N, L]
        e = np.arange(N)[:, None]
        closed = self.ep_end[seq % T, e]
        end = np.where(seq == self.cur_seq[:, None], S - 1, closed)
        return np.clip(end, steps[None, :], S - 1)

    def snapshot(self):
        N, L, S = self.N, self.L, self.S
        assert S > 0
        rows = self.phys(np.arange(N * L))
        data = {k: v[rows] for k, v in self.cols.items()}
        steps = np.arange(S - L, S)
        data['terminals'] = (self.end_steps() == steps[None, :]).astype(np.float32).reshape(-1)
        return data

    def sample(self, cfg, draws, idxs=None):
        """(batch, idxs, value goal idxs, actor goal idxs), indices flat; the
        batch holds the buffer's keys, the goals and the scalars."""
        snap = self.snapshot()
        out, ix, vg, ag = gco.sample(snap, cfg, draws, idxs=idxs)
        if 'terminals' not in self.cols:
            del out['terminals']
        else:  # the buffer's own column holds what was inserted
            out['terminals'] = self.cols['terminals'][self.phys(ix)]
        return out, ix, vg, ag


class Brute:
    """Each env's whole history; the snapshot from the last L entries."""

    def __init__(self, num_envs, horizon):
        self.N, self.T = num_envs, horizon
        self.hist = [[] for _ in range(num_envs)]  # (row dict, done) per step

    def add(self, batch, done):
        for e in range(self.N):
            self.hist[e].append(({k: np.asarray(v)[e] for k, v in batch.items()}, bool(done[e])))

    def snapshot(self, dtypes):
        L = min(len(self.hist[0]), self.T)
        data = {k: [] for k in dtypes}
        term = []
        for e in range(self.N):
            live = self.hist[e][-L:]
            for i, (row, done) in enumerate(live):
                for k in data:
                    data[k].append(row[k])
                term.append(1.0 if (done or i == L - 1) else 0.0)
        out = {k: np.array(v).astype(dtypes[k]) for k, v in data.items()}
        out['terminals'] = np.array(term, np.float32)
        return out


def random_draws(rng, B, npick, max_geom=6):
    """Injected draws over a snapshot of npick rows (names as ogbx_gc_draws)."""
    d = dict(pick=rng.randint(0, npick, B).astype(np.int64))
    for p in ('v_', 'a_'):
        d[p + 'pick'] = rng.randint(0, npick, B).astype(np.int64)
        d[p + 'geom'] = rng.randint(1, max_geom + 1, B).astype(np.int64)
        d[p + 'dist'] = rng.rand(B)
        d[p + 'u_traj'] = rng.rand(B)
        d[p + 'u_cur'] = rng.rand(B)
    return d


def regimes(ring, idxs, vg, draws, cfg, pre='value'):
    """Counts of the sample regimes the tests must reach, from the model alone."""
    p = pre[0] + '_'
    ix = np.asarray(idxs)
    e, k = ring.split(ix)
    steps = ring.S - ring.L + k
    end = ring.end_steps()[e, k]
    open_ep = ring.ep_seq[steps % ring.T, e] == ring.cur_seq[e]
    fin = ix + (end - steps)
    p_cur = cfg[pre + '_p_curgoal']
    is_cur = draws[p + 'u_cur'] < p_cur
    is_traj = ~is_cur & (draws[p + 'u_traj'] < (cfg[pre + '_p_trajgoal'] / (1 - p_cur) if p_cur != 1 else 0))
    is_rand = ~is_cur & ~is_traj
    if cfg[pre + '_geom_sample']:
        clipped = is_traj & (ix + draws[p + 'geom'] > fin)
    else:
        clipped = is_traj & (vg == fin)
    ge, _ = ring.split(vg)
    return dict(clip_open=int((clipped & open_ep).sum()), clip_closed=int((clipped & ~open_ep).sum()),
                success=int((ix == vg).sum()), random_other_env=int((is_rand & (ge != e)).sum()),
                wrapped=int(((ge == e) & (vg > ix) & (ring.phys(vg) < ring.phys(ix))).sum()))
