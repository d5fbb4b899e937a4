"""tests/online_atc_np.py -- TEST INFRASTRUCTURE ONLY.

NumPy restatement of ATC batches over the episode ring
(include/ogbx_online_atc.h, ``GCReplayBuffer.sample_atc``), from the tables of
``online_np.OnlineNp``:

  table(ring, k)        (W, P): W int32 [T, N], the anchors before each live
                        segment of an env, stored like ep_end at
                        (ordinal % T, e); P int64 [N + 1], the exclusive prefix
                        sum over envs of their anchors
  select(ring, W, P, j) pick j of valid(k) -> flat snapshot row, in the closed
                        form the kernel uses (a search over P, then one over
                        the env's live segments in W, then one ep_end entry)
  pick_rows(ring, k)    every pick in order: what ``atc_np.valid_idxs``
                        computes from the snapshot's terminals by compaction
  batch(ring, cfg, k, draws, crop_from)   the expected batch: ``atc_np.batch``
                        over the snapshot without its next_observations

Ordinals differ in uint32, as the insert counts them.  A table slot is the
ordinal mod T as ``OnlineNp`` takes it, of the int32 the ring stores; for every
ordinal below 2^31, and for every T that divides 2^32, that is the kernel's
uint32 remainder.
"""

import numpy as np

import atc_np as anp

U32 = 1 << 32


def _u32(a):
    return np.asarray(a).astype(np.int64) & 0xFFFFFFFF


def _slot(seq, T):
    """Row of ep_end / W of ordinal seq (uint32)."""
    seq %= U32
    return (seq - U32 if seq >= 1 << 31 else seq) % T


def segments(ring, e):
    """(seq0, c, [(b_i, E_i)] for i = 0..c) of env e: its live segments as
    offsets into the L live steps."""
    S, L, T = ring.S, ring.L, ring.T
    t0 = S - L
    seq0 = int(_u32(ring.ep_seq[t0 % T, e]))
    seqn = int(_u32(ring.ep_seq[(S - 1) % T, e]))
    c = min(max((seqn - seq0) % U32, 0), L - 1)
    out, b = [], 0
    for i in range(c):
        E = int(ring.ep_end[_slot(seq0 + i, T), e]) - t0
        E = min(max(E, b), L - 1)
        out.append((b, E))
        b = E + 1
    out.append((b, L - 1))
    return seq0, c, out


def table(ring, k):
    N, T = ring.N, ring.T
    W = np.zeros((T, N), np.int32)
    A = np.zeros(N, np.int64)
    for e in range(N):
        seq0, c, segs = segments(ring, e)
        run = 0
        for i, (b, E) in enumerate(segs):
            W[_slot(seq0 + i, T), e] = run
            run += max(E - b + 1 - k, 0)
        A[e] = run
    return W, np.concatenate([[0], np.cumsum(A)]).astype(np.int64)


def select(ring, W, P, j):
    """Flat snapshot row of every pick in j (each in [0, P[N]))."""
    L, T = ring.L, ring.T
    t0 = ring.S - L
    out = np.empty(len(j), np.int64)
    for n, pick in enumerate(np.asarray(j, np.int64)):
        e = int(np.searchsorted(P, pick, side='right')) - 1  # P[e] <= pick < P[e + 1]
        r = int(pick - P[e])
        seq0 = int(_u32(ring.ep_seq[t0 % T, e]))
        seqn = int(_u32(ring.ep_seq[(ring.S - 1) % T, e]))
        c = min(max((seqn - seq0) % U32, 0), L - 1)
        lo, hi, loads = 0, c, 0
        while lo < hi:  # the largest i with W_i <= r
            m = (lo + hi + 1) // 2
            loads += 1
            if int(W[_slot(seq0 + m, T), e]) <= r:
                lo = m
            else:
                hi = m - 1
        assert loads <= int(np.ceil(np.log2(c + 1)))  # never a walk over the segments
        Wi = int(W[_slot(seq0 + lo, T), e])
        b = 0 if lo == 0 else int(ring.ep_end[_slot(seq0 + lo - 1, T), e]) - t0 + 1
        out[n] = e * L + b + (r - Wi)
    return out


def pick_rows(ring, k):
    W, P = table(ring, k)
    return select(ring, W, P, np.arange(P[-1]))


def dataset(ring):
    """What the reference's ATCDataset sees: the snapshot's observations and
    terminals (next_observations dropped, as frame_stack requires)."""
    snap = ring.snapshot()
    return dict(observations=snap['observations'], terminals=snap['terminals'])


def batch(ring, cfg, k, draws, crop_from=None):
    """(batch in the reference's key order, anchor rows): atc_np.batch over
    the snapshot."""
    return anp.batch(dataset(ring), cfg, k, draws, crop_from)
