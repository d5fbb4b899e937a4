"""tests/online_trl_np.py -- TEST INFRASTRUCTURE ONLY.

NumPy restatement of TRL batches over the episode ring
(include/ogbx_online_trl.h, a ``GCReplayBuffer`` whose config has a TRL agent
name), from the tables of ``online_np.OnlineNp``:

  table(ring)      P, the exclusive prefix sum of the pickable rows per env
  select(ring, P, j)   pick j of the table -> flat snapshot row, in the closed
                   form the kernel uses (a search over P, then one over the
                   env's live closed episodes in ep_end)
  pick_rows(ring)  every pick in order: what ``trl_np.pick_table`` computes
                   from the snapshot's terminals by compaction
  batch(ring, cfg, draws)   the expected batch: ``trl_np.batch`` over the
                   snapshot, with the buffer's own ``terminals`` rule of
                   ``OnlineNp.sample``

Ordinals differ in uint32, as the insert counts them.
"""

import numpy as np

import trl_np as tnp

# the configs of tests/golden/online_trl_golden.npz
CONFIGS = {'geom': tnp.STATE_CFG, 'unif': dict(tnp.STATE_CFG, value_geom_sample=False)}


def _u32(a):
    return np.asarray(a).astype(np.int64) & 0xFFFFFFFF


def _ordinals(ring):
    """(seq0, closed): each env's ordinal at its oldest live row and the
    episodes it closed before its newest row."""
    S, L, T = ring.S, ring.L, ring.T
    seq0 = _u32(ring.ep_seq[(S - L) % T])
    seqn = _u32(ring.ep_seq[(S - 1) % T])
    return seq0, (seqn - seq0) & 0xFFFFFFFF


def table(ring):
    """P int64 [N + 1]; P[N] is the size of the pick table."""
    _, closed = _ordinals(ring)
    V = np.clip(ring.L - 1 - closed, 0, ring.L - 1)
    return np.concatenate([[0], np.cumsum(V)]).astype(np.int64)


def select(ring, P, j):
    """Flat snapshot row of every pick in j (each in [0, P[N]))."""
    N, T, S, L = ring.N, ring.T, ring.S, ring.L
    t0 = S - L
    seq0, closed = _ordinals(ring)
    out = np.empty(len(j), np.int64)
    for n, pick in enumerate(np.asarray(j, np.int64)):
        e = int(np.searchsorted(P, pick, side='right')) - 1  # P[e] <= pick < P[e + 1]
        r = int(pick - P[e])
        lo, hi = 0, int(closed[e])
        while lo < hi:  # the smallest i with G(i) > r
            i = (lo + hi) // 2
            G = int(ring.ep_end[(int(seq0[e]) + i) % (1 << 32) % T, e]) - t0 - i
            if G > r:
                hi = i
            else:
                lo = i + 1
        out[n] = e * L + r + lo
    return out


def pick_rows(ring):
    P = table(ring)
    return select(ring, P, np.arange(P[-1]))


def batch(ring, cfg, draws, idxs=None):
    """(batch in the reference's key order, index vectors) -- trl_np.batch over
    the snapshot.  The batch's ``terminals`` is the buffer's own column (what
    was inserted), absent when the buffer has none."""
    snap = ring.snapshot()
    out, ix = tnp.batch(snap, cfg, draws, idxs=idxs)
    if 'terminals' not in ring.cols:
        del out['terminals']
    else:
        out['terminals'] = ring.cols['terminals'][ring.phys(ix['idxs'])]
    return out, ix


def random_draws(rng, B, ring, cfg, max_geom=6):
    """Injected draws that keep every value goal past its sample: picks over
    the pick table, and a midpoint inside [idx, value goal) computed from the
    restatement itself."""
    import online_np as onp

    P = table(ring)
    d = onp.random_draws(rng, B, int(P[-1]), max_geom)
    d['midpoint'] = np.zeros(B, np.int64)
    _, ix = tnp.batch(ring.snapshot(), cfg, d)
    d['midpoint'] = ix['idxs'] + (rng.rand(B) * (ix['vg'] - ix['idxs'])).astype(np.int64)
    return d
