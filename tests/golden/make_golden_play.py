"""Golden fixture of powderworld play-data collection, from the reference's own
code (tests/golden/play_golden.npz).

Nothing of the reference is copied: behaviors.py and powderworld_env.py are
loaded from the reference tree (make_golden_powder.reference_modules), and the
collection loop is the `main` of data_gen_scripts/generate_powderworld.py
itself, extracted from its source at run time and executed with stand-ins for
what this machine lacks: FLAGS (a namespace), gymnasium.make (a TimeLimit
stand-in around the reference env), trange (range) and np.savez_compressed
(captured, nothing is written).

Every np.random draw of the loop is recorded, per episode and in order, into
the tape layout of include/ogbx_play.h: rand() and the uniform of
choice(agents, p) as themselves, randint as exact floats, choice(elem_names)
as the element's index, shuffle(sides) decomposed into (j3, j2, j1).  The
float32 rand fields of PWSim.forward are recorded separately.

Cases (E episodes of T steps each):
  a  easy    E=2 T=61   p=0.5  observations, actions, terminals, tape
  b  medium  E=2 T=31   p=0.5  the same + rand fields
  c  hard    E=2 T=31   p=0.5  the same + rand fields
  d  (easy)  E=8 T=1001 p=0.5  actions and tape (the forward is skipped)
  e  (easy)  E=8 T=1001 p=0.0  actions and tape (the forward is skipped)
NumPy seeds are searched until the reference alone meets the coverage list
asserted in main().
"""

import ast
import importlib.util
import os
import sys
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_powder as mgp  # noqa: E402
import play_np  # noqa: E402

WORLD = 32
NUM_ELEMS = {'powderworld-easy-v0': 2, 'powderworld-medium-v0': 5, 'powderworld-hard-v0': 8}


def load_reference():
    sim, envm = mgp.reference_modules()
    spec = importlib.util.spec_from_file_location(
        'ogbench.powderworld.behaviors', os.path.join(mgp.REF, 'ogbench/powderworld/behaviors.py'))
    beh = importlib.util.module_from_spec(spec)
    sys.modules['ogbench.powderworld.behaviors'] = beh
    spec.loader.exec_module(beh)
    src = open(os.path.join(mgp.REF, 'data_gen_scripts/generate_powderworld.py')).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'main')
    code = compile(ast.Module(body=[fn], type_ignores=[]), 'generate_powderworld.py:main', 'exec')
    return envm, beh, code


class TimeLimit:
    """gymnasium's TimeLimit, as far as the loop uses it."""

    def __init__(self, env, max_episode_steps, on_reset):
        self.unwrapped, self._max, self._t, self._on_reset = env, max_episode_steps, 0, on_reset

    def reset(self, **kw):
        self._t = 0
        self._on_reset()
        return self.unwrapped.reset(**kw)

    def step(self, action):
        ob, rew, term, trunc, info = self.unwrapped.step(action)
        self._t += 1
        return ob, rew, term, trunc or self._t >= self._max, info


class Recorder:
    """Wraps np.random.{rand, randint, choice, shuffle}; one tape and one list
    of rand fields per episode (a new episode at every env.reset())."""

    def __init__(self):
        self.tapes, self.fields = [], []
        self.elem_names = None

    def new_episode(self):
        self.tapes.append([])
        self.fields.append([])

    def __enter__(self):
        R = np.random
        self._saved = {k: getattr(R, k) for k in ('rand', 'randint', 'choice', 'shuffle')}
        rand, randint, choice, shuffle = (self._saved[k] for k in ('rand', 'randint', 'choice', 'shuffle'))
        tape = lambda: self.tapes[-1]  # noqa: E731

        def w_rand(*shape):
            v = rand(*shape)
            if shape:
                self.fields[-1].append(np.asarray(v).astype(np.float32)[0, 0])  # as PWSim.forward casts them
            else:
                tape().append(float(v))
            return v

        def w_randint(*a, **k):
            v = randint(*a, **k)
            tape().append(float(int(v)))
            return v

        def w_choice(a, p=None):
            if p is None:  # an element name
                v = choice(a)
                tape().append(float(list(a).index(v)))
                return v
            # choice(agents, p): one uniform against the cdf; draw it again from the saved state to record it
            state = np.random.get_state()
            v = choice(a, p=p)
            after = np.random.get_state()
            np.random.set_state(state)
            u = np.random.random_sample()
            same = np.random.get_state()
            assert all(np.array_equal(x, y) for x, y in zip(after, same)), 'choice(p) drew more than one uniform'
            cdf = np.asarray(p, np.float64).cumsum()
            cdf /= cdf[-1]
            assert a[int(cdf.searchsorted(u, side='right'))] is v
            tape().append(float(u))
            return v

        def w_shuffle(x):
            before = list(x)
            shuffle(x)
            perm = [next(i for i, b in enumerate(before) if b is y) for y in x]
            assert len(x) == 4 and sorted(perm) == [0, 1, 2, 3]
            tape().extend(float(j) for j in play_np.js_from_perm(perm))

        R.rand, R.randint, R.choice, R.shuffle = w_rand, w_randint, w_choice, w_shuffle
        return self

    def __exit__(self, *exc):
        for k, fn in self._saved.items():
            setattr(np.random, k, fn)


def run_reference(ref, env_name, episodes, T, p_random, np_seed, simulate=True):
    """generate_powderworld.main with stand-ins; returns (dataset, tapes, fields)."""
    envm, beh, code = ref
    rec = Recorder()

    def make(name, mode, max_episode_steps):
        env = envm.PowderworldEnv(world_size=WORLD, num_elems=NUM_ELEMS[name], mode=mode)
        if not simulate:
            # actions-only cases: the world and its render play no part in the actions
            env.pw.forward = lambda world: world
            env._get_ob = lambda: np.zeros(1, np.uint8)
        return TimeLimit(env, max_episode_steps, rec.new_episode)

    saved = {}
    flags = types.SimpleNamespace(seed=0, env_name=env_name, dataset_type='play', save_path='/nonexistent/play.npz',
                                  num_episodes=episodes, max_episode_steps=T, p_random_action=p_random)
    pathlib = types.SimpleNamespace(Path=lambda p: types.SimpleNamespace(
        parent=types.SimpleNamespace(mkdir=lambda **k: None)))
    ns = dict(FLAGS=flags, gymnasium=types.SimpleNamespace(make=make), np=np, trange=range, pathlib=pathlib,
              defaultdict=defaultdict, FillBehavior=beh.FillBehavior, LineBehavior=beh.LineBehavior,
              SquareBehavior=beh.SquareBehavior, print=lambda *a: None)
    exec(code, ns)
    real_save = np.savez_compressed
    np.savez_compressed = lambda path, **arrays: saved.__setitem__(path, arrays)
    np.random.seed(np_seed)
    try:
        with rec:
            ns['main'](None)
    finally:
        np.savez_compressed = real_save
    data = saved['/nonexistent/play.npz']
    assert len(saved['/nonexistent/play-val.npz']['actions']) == 0
    # the first env.reset() precedes the loop: its (empty) episode is dropped
    assert rec.tapes[0] == [] and len(rec.tapes) == episodes + 1
    return data, rec.tapes[1:], rec.fields[1:]


def coverage(tapes, T, num_elems, p_random, size):
    """What the episodes of one case exercise (from the tapes alone)."""
    got = set()
    for tp in tapes:
        behs = []
        _, used, recs = play_np.plan_episode(tp, T, size, num_elems, p_random, behaviors=behs)
        assert used == len(tp)
        for b in behs:
            got.add(('kind', b.kind))
            if b.kind == play_np.SQUARE:
                length, _, _, rev, perm = b.args
                got.add(('square_len', 'one' if length == 1 else 'max' if length == size - 1 else 'mid'))
                if rev:
                    got.add('reversed')
                if perm != [0, 1, 2, 3]:
                    got.add('shuffled')
            if b.kind == play_np.FILL and b.finished_at is not None:
                got.add('fill_done')  # run to completion and replaced
            if b.finished_at == len(recs) - 1:
                got.add('done_at_last_decision')
    return got


WANT = {('kind', 0), ('kind', 1), ('kind', 2), 'fill_done', ('square_len', 'one'), ('square_len', 'max'), 'reversed',
        'shuffled', 'done_at_last_decision'}


def main():
    ref = load_reference()
    size = WORLD // 4
    out, got = {}, set()
    cases = [('a', 'powderworld-easy-v0', 2, 61, 0.5, True), ('b', 'powderworld-medium-v0', 2, 31, 0.5, True),
             ('c', 'powderworld-hard-v0', 2, 31, 0.5, True), ('d', 'powderworld-easy-v0', 8, 1001, 0.5, False),
             ('e', 'powderworld-easy-v0', 8, 1001, 0.0, False)]
    for name, env_name, E, T, p, simulate in cases:
        ne = NUM_ELEMS[env_name]
        np_seed = 7000 + ord(name)
        while True:
            data, tapes, fields = run_reference(ref, env_name, E, T, p, np_seed, simulate)
            cov = coverage(tapes, T, ne, p, size)
            # the long cases carry the coverage list: search their seeds
            # (e cannot end a behaviour at its last decision: with p = 0 every
            # decision is an entry, every sequence length is a multiple of 4 at
            # size 8, and an episode of 1001 steps has 334 decisions)
            if simulate or WANT - {'fill_done' if name == 'd' else 'done_at_last_decision'} <= cov:
                break
            print(f'case {name}: numpy seed {np_seed} lacks {sorted(map(str, WANT - cov))}', flush=True)
            np_seed += 1
        got |= cov
        print(f'case {name}: numpy seed {np_seed}, tape lengths {[len(t) for t in tapes]}, coverage {sorted(map(str, cov))}')
        acts = np.asarray(data['actions'], np.int32)
        assert acts.shape == (E * T,)
        for e, tp in enumerate(tapes):  # the restatement replays the reference exactly
            a, used, _ = play_np.plan_episode(tp, T, size, ne, p)
            assert used == len(tp) and np.array_equal(a, acts[e * T:(e + 1) * T]), (name, e)
        L = max(len(t) for t in tapes)
        tape = np.zeros((E, L), np.float64)
        for e, tp in enumerate(tapes):
            tape[e, :len(tp)] = tp
        out[f'{name}_meta'] = np.array([E, T, ne, WORLD], np.int64)
        out[f'{name}_p_random'] = np.array(p, np.float64)
        out[f'{name}_actions'] = acts
        out[f'{name}_tape'] = tape
        out[f'{name}_tape_len'] = np.array([len(t) for t in tapes], np.int32)
        if simulate:
            out[f'{name}_obs'] = np.asarray(data['observations'], np.uint8)
            out[f'{name}_terminals'] = np.asarray(data['terminals']).astype(bool)
            assert out[f'{name}_obs'].shape == (E * T, WORLD, WORLD, 6)
            if ne != 2:
                # [E, forwards, 3, H, W]: forward q of an episode is the one of step 3q + 2
                F = T // 3
                assert all(len(f) == 3 * F for f in fields)
                out[f'{name}_rand'] = np.stack([np.stack(f).reshape(F, 3, WORLD, WORLD) for f in fields])
    assert WANT <= got, f'coverage missing: {WANT - got}'
    path = os.path.join(HERE, 'play_golden.npz')
    np.savez_compressed(path, **out)
    print('play golden:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
