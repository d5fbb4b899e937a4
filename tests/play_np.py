"""NumPy restatement of the powderworld play policy's action plan
(include/ogbx_play.h): the episode state machine, the closed-form behaviour
sequences, the Fisher-Yates decomposition of the side order and the tape of
injected draws.  Test infrastructure: the CPU tests replay the reference's
recorded draws through it, the GPU tests compare the kernel with the same
fixtures.

A tape is the sequence of values the collection loop draws for one env, in the
order it draws them: uniforms as themselves, integers as exact floats, an
element as its index, a shuffle of the four sides as (j3, j2, j1).
"""

import numpy as np

FILL, LINE, SQUARE = 0, 1, 2
WEIGHTS = (1.0, 3.0, 3.0)


def behavior_cdf(weights=WEIGHTS):
    p = np.asarray(weights, np.float64)
    cdf = (p / p.sum()).cumsum()
    return cdf / cdf[-1]


# ------------------------------------------------------------ side order
def perm_from_js(j3, j2, j1):
    """Order of four items after a top-down Fisher-Yates with these picks:
    position q of the result holds item perm[q]."""
    perm = [0, 1, 2, 3]
    for i, j in ((3, j3), (2, j2), (1, j1)):
        perm[i], perm[j] = perm[j], perm[i]
    return perm


def js_from_perm(perm):
    """The picks (j3, j2, j1) that produce `perm`: undo the swaps from the top."""
    cur = [0, 1, 2, 3]
    js = []
    for i in (3, 2, 1):
        j = cur.index(perm[i])  # the item that ends at position i was at j <= i
        assert j <= i
        cur[i], cur[j] = cur[j], cur[i]
        js.append(j)
    return tuple(js)


# ------------------------------------------------------------ sequences
def fill_entry(i, size, flip_x, flip_y, flip_xy):
    x, y = i % size, i // size
    if flip_x:
        x = size - 1 - x
    if flip_y:
        y = size - 1 - y
    return (y, x) if flip_xy else (x, y)


def line_entry(i, size, target, flip_dir, flip_xy):
    x, y = i, (size - 1 - target if flip_dir else target)
    return (y, x) if flip_xy else (x, y)


def square_entry(s, length, x1, y1, rev, perm):
    """rev: reverse bit of side k at bit k; perm: side of each quarter."""
    q, o = divmod(s, length + 1)
    side = perm[q]
    if (rev >> side) & 1:
        o = length - o
    if side == 0:
        return x1, y1 + o
    if side == 1:
        return x1 + length, y1 + o
    if side == 2:
        return x1 + o, y1
    return x1 + o, y1 + length


class Behavior:
    """One behaviour after its reset draws; entry(i) is its i-th (x, y)."""

    def __init__(self, pop, cdf, size, num_elems):
        u = pop()
        self.kind = min(int(np.searchsorted(cdf, u, side='right')), 2)
        self.elem = int(pop())
        self.size, self.step = size, 0
        self.finished_at = None  # the decision at which it was done and replaced
        if self.kind == FILL:
            self.args = tuple(int(pop()) for _ in range(3))
            self.count = size * size
        elif self.kind == LINE:
            self.args = tuple(int(pop()) for _ in range(3))
            self.count = size
        else:
            length, x1, y1 = int(pop()), int(pop()), int(pop())
            rev = sum(int(pop()) << k for k in range(4))
            perm = perm_from_js(int(pop()), int(pop()), int(pop()))
            self.args = (length, x1, y1, rev, perm)
            self.count = 4 * (length + 1)

    def entry(self, i):
        if self.kind == FILL:
            return fill_entry(i, self.size, *self.args)
        if self.kind == LINE:
            return line_entry(i, self.size, *self.args)
        return square_entry(i, *self.args)


# ------------------------------------------------------------ the episode
def plan_episode(tape, T, size, num_elems, p_random, cdf=None, behaviors=None):
    """Actions of one env's episode of T steps from its tape.

    Returns (actions int32 [T], used, records): used = values consumed,
    records = one (random, kind, fresh, index) per decision.  behaviors: a
    list that receives every Behavior of the episode, in order."""
    cdf = behavior_cdf() if cdf is None else cdf
    pos = [0]

    def pop():
        v = tape[pos[0]]
        pos[0] += 1
        return v

    behaviors = [] if behaviors is None else behaviors
    beh = Behavior(pop, cdf, size, num_elems)
    behaviors.append(beh)
    fresh = True
    actions = np.zeros(T, np.int32)
    records = []
    held = (0, 0, 0)
    for t in range(T):
        stage = t % 3
        if stage == 0:
            random = pop() < p_random
            records.append((bool(random), beh.kind, fresh, beh.step))
            fresh = False
            if random:
                held = (int(pop()), int(pop()), int(pop()))
            else:
                x, y = beh.entry(beh.step)
                held = (beh.elem, x, y)
                beh.step += 1
        actions[t] = held[stage]
        # the done check of every step; only a decision can finish a behaviour
        if beh.step == beh.count:
            beh.finished_at = t // 3
            beh = Behavior(pop, cdf, size, num_elems)
            behaviors.append(beh)
            fresh = True
    return actions, pos[0], records


def plan(tapes, T, size, num_elems, p_random, cdf=None):
    """plan_episode for every row of tapes [N, L]: (actions [T, N], used [N])."""
    res = [plan_episode(tp, T, size, num_elems, p_random, cdf) for tp in tapes]
    return np.stack([r[0] for r in res], 1), np.array([r[1] for r in res], np.int32)


def pack_record(rec):
    """The kernel's decision word of a plan_episode record."""
    random, kind, fresh, index = rec
    return int(random) | (kind << 1) | (int(fresh) << 3) | (index << 8)
