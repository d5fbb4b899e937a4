"""Host model of powderworld's Philox streams, written from the documented
layout (INTEGRATION.md "Powderworld streams"; the fill_rands comment of
ogbench_amd/csrc/powder_full.h; the OGBX_STREAM_VERSION note of
include/ogbx.h), not from values read back from a GPU.

  * Philox4x32-10 in NumPy (uint64 arithmetic over arrays of counters).
  * key(seed, tag) = (lo32(seed), hi32(seed) ^ tag), tags 0x50570001 (reset),
    0x50570002 (action), 0x50570003 (rand).
  * draw(seed, tag, env, ep, slot, bound): word 0 of counter (lo32(env), ep,
    slot, hi32(env)), reduced by (w * bound) >> 32.
  * rand_fields(seed, env, ep, slot, H): float32 [3, H, H].  The cells of a
    column whose rows are congruent mod H/4 form a group of four; group (r, c),
    r < H/4, has index g = r*H + c and takes the 12 words of the three calls at
    counter (4g + k, lo32(env), ep, slot), k = 0..2, under the rand key with
    word 0 xor hi32(env).  Member j (row r + j*H/4) takes words 3j, 3j+1, 3j+2
    as (rand_movement, rand_interact, rand_element), each (w >> 8) * 2^-24.
  * slots of the fields: (1<<24) | q for goal-replay forward q, 2<<24 for the
    reset's forward, (3<<24) | elapsed for a step's forward.

Limit this rests on: the purpose of a field slot is OR-ed into bits 24-25, so
the counters of one env-episode are distinct only while ``elapsed`` and the
goal index stay below 2^24.

PhiloxEnv replays one env of a Philox-mode run around the NumPy oracles
(oracle/powder_np.py, oracle/powder_full_np.py); scenario() defines, once, the
runs that tests/test_powder_philox_cpu.py checks for sensitivity and
tests/test_powder_philox_gpu.py replays on the device.
"""

import collections
import functools

import numpy as np

from ogbench_amd.powder_tasks import task_sequences, task_tols
from oracle import powder_full_np as pwf
from oracle import powder_np as pw
from powder_worlds import seeded_world

M32 = np.uint64(0xFFFFFFFF)
TAG_RESET, TAG_ACTION, TAG_RAND = 0x50570001, 0x50570002, 0x50570003
RAND_GOAL, RAND_START, RAND_STEP = 1 << 24, 2 << 24, 3 << 24
NUM_ELEMS = {'easy': 2, 'medium': 5, 'hard': 8}


def philox4x32(ctr, key):
    """Philox4x32-10.  ctr [..., 4], key [..., 2] (broadcast against each
    other) -> uint32 [..., 4]."""
    ctr, key = np.asarray(ctr, np.uint64), np.asarray(key, np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape) for i in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape), np.broadcast_to(key[..., 1], shape)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & M32, (p0 >> s32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def lo32(v):
    return int(v) & 0xFFFFFFFF


def hi32(v):
    return (int(v) >> 32) & 0xFFFFFFFF


def key(seed, tag):
    return lo32(seed), hi32(seed) ^ tag


def draw_counter(env, ep, slot):
    return lo32(env), int(ep), int(slot), hi32(env)


def draw(seed, tag, env, ep, slot, bound):
    w = int(philox4x32(draw_counter(env, ep, slot), key(seed, tag))[0])
    return (w * int(bound)) >> 32


# A layout names how the fields are cut from the stream.  RIGHT is the
# documented one; the others are the near misses the scenarios must notice.
Layout = collections.namedtuple('Layout', 'channel_shift slot_shift adjacent_rows')
RIGHT = Layout(0, 0, False)
WRONG_LAYOUTS = {
    'channels_rotated': Layout(1, 0, False),
    'slot_off_by_one': Layout(0, 1, False),
    'adjacent_rows': Layout(0, 0, True),
}


def field_counters(seed, env, ep, slot, H):
    """(counters uint64 [H/4, H, 3, 4], key (k0, k1)) of one forward's fields."""
    r, c = np.meshgrid(np.arange(H // 4), np.arange(H), indexing='ij')
    g = (r * H + c).astype(np.uint64)
    ctr = np.zeros((H // 4, H, 3, 4), np.uint64)
    for k in range(3):
        ctr[:, :, k, 0] = np.uint64(4) * g + np.uint64(k)
    ctr[..., 1], ctr[..., 2], ctr[..., 3] = lo32(env), int(ep), int(slot)
    k0, k1 = key(seed, TAG_RAND)
    return ctr, (k0 ^ hi32(env), k1)


def rand_fields(seed, env, ep, slot, H, layout=RIGHT):
    """float32 [3, H, H]: rand_movement, rand_interact, rand_element."""
    ctr, k = field_counters(seed, env, ep, slot + layout.slot_shift, H)
    words = philox4x32(ctr, k).reshape(H // 4, H, 12)
    out = np.zeros((3, H, H), np.float32)
    r = np.arange(H // 4)
    for j in range(4):
        rows = 4 * r + j if layout.adjacent_rows else r + j * (H // 4)
        for ch in range(3):
            out[ch, rows, :] = (words[:, :, 3 * j + ch] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.roll(out, layout.channel_shift, axis=0)


@functools.lru_cache(maxsize=None)
def easy_goal(size, task):
    """Goal ids of an easy task: its sequence replayed from the blank world
    (deterministic: the easy rules draw nothing)."""
    o = pw.Env(size)
    st = o.blank()
    for e, x, y in task_sequences(2)[task - 1]:
        st = pw.paint(*pw.forward(*st), pw.EASY_ELEMS[e], x, y)
    return st[0]


@functools.lru_cache(maxsize=None)
def goal_world(layout, ne, size, seed, env, ep, task):
    """Goal world of a medium/hard episode: the task's sequence replayed from
    the blank world, forward q under the fields of slot (1<<24) | q.  Kept per
    process: scenarios that start alike share their replays."""
    seq = task_sequences(ne)[task - 1]
    gw = pwf.Env(ne, size).replay(seq, [rand_fields(seed, env, ep, RAND_GOAL | q, size, layout) for q in range(len(seq))])
    gw.setflags(write=False)
    return gw


class PhiloxEnv:
    """One env of a Philox-mode run: env index ``env`` (env_base included) of a
    handle seeded ``seed``.  step() follows the kernels: success is errors <
    tol of the current world at every step, truncated is elapsed >=
    max_episode_steps, and with auto_reset the same step returns the next
    episode's first observation (same task, episode + 1, draws 1..3)."""

    def __init__(self, env_type, size, seed, env, max_episode_steps=500, auto_reset=False, layout=RIGHT):
        self.ne = NUM_ELEMS[env_type]
        self.full = self.ne != 2
        self.size, self.seed, self.env, self.layout = size, int(seed), int(env), layout
        self.xy = (size - 4) // 4 + 1
        self.max_steps, self.auto_reset = max_episode_steps, auto_reset
        self.seqs, self.tols = task_sequences(self.ne), task_tols(self.ne)
        self.o = pwf.Env(self.ne, size) if self.full else pw.Env(size)
        self.episode = self.elapsed = self.task = 0
        self.ctrl_elem = self.ctrl_x = 0
        self.succ = False
        self.replaced = [0, 0, 0]  # invalid actions replaced, by stage
        self.auto_resets = 0

    def fields(self, ep, slot):
        return rand_fields(self.seed, self.env, ep, slot, self.size, self.layout)

    def _errors(self):
        return self.o.errors() if self.full else pw.error_count(self.o.state[0], self.o.goal)

    def _begin(self, ep):
        """Episode ``ep`` of the current task: goal, blank world, the drawn
        initial action.  Returns the first observation."""
        e, x, y = (draw(self.seed, TAG_RESET, self.env, ep, s, b) for s, b in ((1, self.ne), (2, self.xy), (3, self.xy)))
        self.goal_obs = np.zeros((self.size, self.size, 6), np.uint8)
        if self.full:
            gw = goal_world(self.layout, self.ne, self.size, self.seed, self.env, ep, self.task)
            self.goal_obs[..., :3] = pwf.render(gw[0])
            ob = self.o.reset(gw[0, 0].astype(np.uint8), e, x, y, self.fields(ep, RAND_START))
        else:
            goal = easy_goal(self.size, self.task)
            self.goal_obs[..., :3] = pw.render_lut()[goal]
            ob = self.o.reset(goal, e, x, y)
        self.episode, self.elapsed = ep, 0
        self.succ = self._errors() < self.tols[self.task - 1]
        return ob

    def reset(self, task_id=None):
        """Returns (obs, goal obs).  task_id None: drawn at slot 0."""
        ep = self.episode + 1
        self.task = task_id if task_id is not None else 1 + draw(self.seed, TAG_RESET, self.env, ep, 0, len(self.seqs))
        self.ctrl_elem = self.ctrl_x = 0
        return self._begin(ep), self.goal_obs

    def reseed(self, seed):
        self.seed, self.episode = int(seed), 0

    @property
    def stage(self):
        return self.o.stage

    def step(self, a):
        """(obs, reward, terminated, truncated, success) of one env step."""
        stage = self.o.stage
        bound = self.ne if stage == 0 else self.xy
        if not 0 <= a < bound:
            a = draw(self.seed, TAG_ACTION, self.env, self.episode, self.elapsed, bound)
            self.replaced[stage] += 1
        if stage == 0:
            self.ctrl_elem = a
        elif stage == 1:
            self.ctrl_x = a
        if self.full:
            ob = self.o.step(a, self.fields(self.episode, RAND_STEP | self.elapsed) if stage == 2 else None)
        else:
            ob = self.o.step(a)[0]
        if stage == 2:
            self.succ = self._errors() < self.tols[self.task - 1]
        self.elapsed += 1
        succ, trunc = self.succ, self.elapsed >= self.max_steps
        if self.auto_reset and (succ or trunc):
            ob = self._begin(self.episode + 1)
            self.auto_resets += 1
        return ob, np.float32(succ), succ, trunc, succ

    @property
    def ctrl(self):
        return self.o.stage | self.ctrl_elem << 2 | self.ctrl_x << 8 | self.task << 16 | int(self.succ) << 24

    def world(self):
        """medium/hard: the (9, H, W) float32 world; easy: the packed bytes."""
        if self.full:
            return self.o.w[0]
        ids, grav, didg = self.o.state
        return (ids | grav << 5 | didg << 6).astype(np.uint8)

    def goal_ids(self):
        return np.asarray(self.o.goal, np.uint8)


# ---------------------------------------------------------------- scenarios
# A scenario is a handle's configuration and a program of host calls:
#   ('reset', seed or None, task ids [n] or None, mask [n] or None)
#   ('step', actions [n])
#   ('phase', p)      a set_step_phase hint: the device only, results unchanged
Scenario = collections.namedtuple('Scenario', 'name env_type size n env_base max_episode_steps auto_reset program')
Step = collections.namedtuple('Step', 'obs reward terminated truncated success stage')  # stage: before the step
Reset = collections.namedtuple('Reset', 'obs goal mask')


def _actions(rng, ne, xy, steps, n):
    """Random actions, some invalid at every stage (negative, at the bound and
    above it)."""
    return rng.randint(-2, max(ne, xy) + 3, size=(steps, n))


def _steps(acts):
    return [('step', [int(v) for v in a]) for a in acts]


def _in_phase(name, env_type, size, n, tasks, max_steps, steps, seed, rs):
    ne = NUM_ELEMS[env_type]
    acts = _actions(np.random.RandomState(rs), ne, (size - 4) // 4 + 1, steps, n)
    return Scenario(name, env_type, size, n, 0, max_steps, True, [('reset', seed, tasks, None)] + _steps(acts))


def _out_of_phase(name, env_type, size, n, tasks, max_steps, steps, seed, rs, hint):
    """Reset, step, re-reset env 0, step, re-reset env 1: stages 1, 0 and 2 side
    by side from then on (the sparse and the light kernel in one step), with one
    wrong phase hint on the way."""
    ne = NUM_ELEMS[env_type]
    acts = _actions(np.random.RandomState(rs), ne, (size - 4) // 4 + 1, steps + 2, n)
    m0, m1 = [int(i == 0) for i in range(n)], [int(i == 1) for i in range(n)]
    st = _steps(acts)
    prog = [('reset', seed, tasks, None), st[0], ('reset', None, tasks, m0), st[1], ('reset', None, tasks, m1)]
    prog += st[2:5] + [('phase', hint)] + st[5:]
    return Scenario(name, env_type, size, n, 0, max_steps, True, prog)


def _own_sequence(name, env_type, size, task, seed, more=12):
    """One env (index = task) plays its task's own action sequence until the
    model reports success, then ``more`` steps into the next episode."""
    seq = task_sequences(NUM_ELEMS[env_type])[task - 1]
    flat = [v for a in seq for v in a]
    env = PhiloxEnv(env_type, size, seed, task, 500, True)
    env.reset(task)
    t_succ = next(t for t, a in enumerate(flat) if env.step(a)[2])
    prog = [('reset', seed, [task], None)] + [('step', [a]) for a in (flat + flat)[:t_succ + 1 + more]]
    return Scenario(name, env_type, size, 1, task, 500, True, prog), t_succ


SEED = 11

_BUILDERS = {
    # single steps in phase (and, from the same start, the fused rollout)
    'medium32': lambda: _in_phase('medium32', 'medium', 32, 4, [1, 4, 1, 4], 7, 15, SEED, 1),
    'hard32': lambda: _in_phase('hard32', 'hard', 32, 4, [3, 2, 3, 2], 7, 15, SEED, 2),
    'medium64': lambda: _in_phase('medium64', 'medium', 64, 3, [1, 4, 1], 7, 15, SEED, 3),
    'easy32': lambda: _in_phase('easy32', 'easy', 32, 5, [1, 2, 3, 4, 5], 7, 30, SEED, 4),
    'easy64': lambda: _in_phase('easy64', 'easy', 64, 5, [5, 4, 3, 2, 1], 7, 30, SEED, 5),
    # single steps out of phase
    'medium32_mixed': lambda: _out_of_phase('medium32_mixed', 'medium', 32, 4, [1, 4, 1, 4], 7, 15, SEED, 6, 1),
    'hard32_mixed': lambda: _out_of_phase('hard32_mixed', 'hard', 32, 4, [3, 2, 3, 2], 7, 15, SEED, 7, 0),
    # env indices on both sides of 2^32
    'medium32_env64': lambda: Scenario(
        'medium32_env64', 'medium', 32, 4, 2 ** 32 - 2, 500, False,
        [('reset', SEED, [1, 4, 1, 4], None)] + _steps(_actions(np.random.RandomState(8), 5, 8, 12, 4))),
}
# resets: 6 envs, env_base 0, the task given or drawn at slot 0
for _t in ('easy', 'medium', 'hard'):
    _given = {'easy': [1, 2, 3, 4, 5, 1], 'medium': [1, 4, 1, 4, 5, 2], 'hard': [3, 2, 3, 2, 1, 4]}[_t]
    _BUILDERS[f'reset_{_t}_given'] = lambda t=_t, g=_given: Scenario(
        f'reset_{t}_given', t, 32, 6, 0, 500, False, [('reset', SEED, g, None)])
    _BUILDERS[f'reset_{_t}_drawn'] = lambda t=_t: Scenario(
        f'reset_{t}_drawn', t, 32, 6, 0, 500, False, [('reset', SEED, None, None)])
_OWN = {'medium32_task3': ('medium', 32, 3), 'hard32_task4': ('hard', 32, 4),
        'easy32_task1': ('easy', 32, 1), 'easy64_task3': ('easy', 64, 3)}

STEP_SCENARIOS = ['medium32', 'hard32', 'medium64', 'medium32_mixed', 'hard32_mixed']
EASY_SCENARIOS = ['easy32', 'easy64']
RESET_SCENARIOS = [f'reset_{t}_{k}' for t in ('easy', 'medium', 'hard') for k in ('given', 'drawn')]
OWN_SCENARIOS = list(_OWN)
# the scenarios whose trajectories depend on the rand fields (medium/hard)
FIELD_SCENARIOS = (STEP_SCENARIOS + ['medium32_env64'] + [s for s in RESET_SCENARIOS if 'easy' not in s]
                   + [s for s in OWN_SCENARIOS if 'easy' not in s])


@functools.lru_cache(maxsize=None)
def _own(name):
    return _own_sequence(name, *_OWN[name], seed=SEED)


@functools.lru_cache(maxsize=None)
def scenario(name):
    return _own(name)[0] if name in _OWN else _BUILDERS[name]()


def success_step(name):
    """Index of the step of an own-sequence scenario at which the model succeeds."""
    return _own(name)[1]


def make_envs(sc, layout=RIGHT, only=None):
    return [PhiloxEnv(sc.env_type, sc.size, 0, sc.env_base + i, sc.max_episode_steps, sc.auto_reset, layout)
            if only is None or i == only else None for i in range(sc.n)]


def run_program(sc, envs):
    """Generator over the program's records (Reset / Step of per-env lists,
    None for envs not run or not reset); 'phase' ops yield nothing."""
    for op in sc.program:
        if op[0] == 'reset':
            _, seed, tasks, mask = op
            obs, goal = [None] * sc.n, [None] * sc.n
            for i, e in enumerate(envs):
                if e is None or (mask is not None and not mask[i]):
                    continue
                if seed is not None:
                    e.reseed(seed)
                obs[i], goal[i] = e.reset(None if tasks is None else tasks[i])
                goal[i] = goal[i].copy()
            yield Reset(obs, goal, mask)
        elif op[0] == 'step':
            stage = [None if e is None else e.stage for e in envs]
            outs = [None if e is None else e.step(op[1][i]) for i, e in enumerate(envs)]
            yield Step(*([None if o is None else o[k] for o in outs] for k in range(5)), stage)


Trajectory = collections.namedtuple('Trajectory', 'records envs')


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """The right model's records of a scenario and its envs at the end (computed
    once per process: the CPU and the GPU tests share it)."""
    sc = scenario(name)
    envs = make_envs(sc)
    return Trajectory(list(run_program(sc, envs)), envs)


def first_difference(name, layout, env):
    """Index of the first record of env ``env`` whose compared observation
    differs between the right model and ``layout``, or None.  A scenario with
    steps counts its step observations alone (a goal observation that differs
    says nothing about the step slots); a reset scenario counts the first and
    the goal observation.  Stops at the difference: what follows costs oracle
    forwards and cannot undo it."""
    sc = scenario(name)
    right = trajectory(name).records
    has_steps = any(op[0] == 'step' for op in sc.program)
    for k, rec in enumerate(run_program(sc, make_envs(sc, layout, only=env))):
        ref = right[k]
        if rec.obs[env] is None or (has_steps and isinstance(rec, Reset)):
            continue
        if not np.array_equal(rec.obs[env], ref.obs[env]):
            return k
        if isinstance(rec, Reset) and not np.array_equal(rec.goal[env], ref.goal[env]):
            return k
    return None


def forward_worlds(size, n=3, ne=8):
    """The seeded worlds of the forward_full cases (every element of the set)."""
    return seeded_world(np.random.RandomState(200 + size), n, size, ne)


def forward_full_model(w, seed, steps, layout=RIGHT, chained=True):
    """forward_full without rand: env = world index, episode 0, slot (3<<24) | q
    with q the forward's index inside its call."""
    w = np.array(w, np.float32)
    H = w.shape[-1]
    for t in range(steps):
        f = np.stack([rand_fields(seed, e, 0, RAND_STEP | (t if chained else 0), H, layout) for e in range(len(w))])
        w = pwf.forward(w, [f[:, c] for c in range(3)])
    return w
