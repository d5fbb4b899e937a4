"""Golden fixture for the dataset ingest path, from the reference's own code.

Calls the reference's ogbench/utils.py load_dataset and
ogbench/relabel_utils.py relabel_dataset / add_oracle_reps (imported the way
make_golden_gc.py imports them) on small designed raw files and saves inputs
and outputs only (tests/golden/ingest_golden.npz).

Raw files.  Three families whose rows are sized to reach every lane width of
ogbx_gather_rows, with a terminal layout that is spelt out below (not drawn):

  ant     263 rows  observations f32 [29], actions f32 [8], qpos f64 [15],
                    qvel f64 [14], button_states uint8 [5]
  visual  263 rows  observations uint8 [4,4,3] (ob_dtype=uint8), actions f32 [2]
  powder  257 rows  observations uint8 [3,3,3], actions int32 1-D
                    (action_dtype=int32)
  one       1 row   the ant columns; its only row is terminal

Each is loaded compact / regular, with and without add_info.  A raw column is
stored once (raw_<family>_<column>); an expected column is stored only where it
differs from the raw one (exp_<family>_<mode>_<column>); the key order, dtypes
and shapes of every load go into keys_<family>_<mode>_<info|noinfo> as strings
"key|dtype|d0,d1,...".

Relabel boundary block (rb_*).  For qpos in f32 and f64: 2,048 rows around a
goal with no short binary expansion.  The reference decides success with
sqrt(dx*dx + dy*dy) <= tol in float64; a build that contracts the sum into
fma(dx, dx, dy*dy) or fma(dy, dy, dx*dx) rounds once less and moves the
distance by an ulp on about 8 % of rows.  K = 32 such rows are picked: for the
first 16 the plain distance is the smaller one, for the other 16 the larger.
Call k runs the reference with _goal_tol = the plain distance of row k, so row
k sits exactly on `<=`:

  rb_<dt>_succ [32, 2048]  success of call k (rewards = succ - 1, masks = 1 - succ)

With that tolerance a contracted form can only change row k where the plain
distance is the smaller one (the row fails).  Where it is the larger one the
contracted distance is still <= tol, so for those 16 rows there is a second
call whose tolerance is the contracted distance of row k (the largest one
below the plain distance); there the reference fails row k and a contracted
build adds a success:

  rb_<dt>_succ_below [16, 2048]

ant_relabel_succ [263] is the reference on the ant family's qpos (stride 15).
"""

import io
import math
import os
import sys
import tempfile
import zipfile
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_gc import reference_modules  # noqa: E402

# Trajectory lengths, in file order; the last row of each is terminal.  `tail`
# rows follow the last trajectory with no terminal at all.
#   row 0 terminal (length 1), two more length-1 trajectories, lengths 2, 63,
#   64, 65, then one trajectory that runs across row 256.
LAYOUT = {
    'ant': dict(lengths=[1, 1, 1, 2, 63, 64, 65, 62, 4], tail=0),      # rows 197..258 hold row 256
    'visual': dict(lengths=[1, 1, 1, 2, 63, 64, 65, 62], tail=4),     # last 4 rows: no terminal
    'powder': dict(lengths=[1, 1, 1, 2, 63, 64, 65, 60], tail=0),     # rows 197..256, file ends there
    'one': dict(lengths=[1], tail=0),
}
ROWS = {'ant': 263, 'visual': 263, 'powder': 257, 'one': 1}
LOAD_KW = {
    'ant': {},
    'visual': dict(ob_dtype=np.uint8),
    'powder': dict(ob_dtype=np.uint8, action_dtype=np.int32),
    'one': {},
}
RB_ROWS, RB_K = 2048, 32
RB_GOAL = np.array([12.3, -4.7])
ANT_GOAL, ANT_TOL = np.array([1.3, -0.7]), 4.0


def terminals_of(family):
    lay = LAYOUT[family]
    t = []
    for L in lay['lengths']:
        t += [0.0] * (L - 1) + [1.0]
    t += [0.0] * lay['tail']
    return np.array(t, np.float32)


def _coarse(rng, shape, dtype):
    """Floats on a 1/256 grid in [-8, 8): exact in float32, and few enough
    distinct values that the compressed file stays small."""
    return (rng.randint(-2048, 2048, shape) / 256.0).astype(dtype)


def raw_columns(family, rng):
    n = ROWS[family]
    t = terminals_of(family)
    assert len(t) == n, (family, len(t))
    if family in ('ant', 'one'):
        return dict(observations=_coarse(rng, (n, 29), np.float32), actions=_coarse(rng, (n, 8), np.float32),
                    terminals=t, qpos=_coarse(rng, (n, 15), np.float64), qvel=_coarse(rng, (n, 14), np.float64),
                    button_states=rng.randint(0, 256, (n, 5)).astype(np.uint8))
    if family == 'visual':
        return dict(observations=rng.randint(0, 256, (n, 4, 4, 3)).astype(np.uint8),
                    actions=_coarse(rng, (n, 2), np.float32), terminals=t)
    return dict(observations=rng.randint(0, 256, (n, 3, 3, 3)).astype(np.uint8),
                actions=rng.randint(0, 8, n).astype(np.int32), terminals=t)


def check_layout(family, t):
    """The designed counts, asserted before anything is written."""
    n = len(t)
    locs = np.nonzero(t)[0]
    lengths = np.diff(np.concatenate([[-1], locs]))
    assert n == ROWS[family] and n % 64 != 0 and n % 256 != 0
    assert t[0] == 1, 'row 0 is terminal'
    if family == 'one':
        assert n == 1
        return
    assert list(lengths[:3]) == [1, 1, 1], 'three length-1 trajectories, adjacent terminals'
    assert list(lengths[3:7]) == [2, 63, 64, 65]
    start, end = locs[6] + 1, locs[7]
    assert start < 256 <= end, 'one trajectory runs across row 256'
    assert (t[-1] == 1) == (family != 'visual'), 'ant and powder end on a terminal, visual does not'
    assert lengths.tolist() == LAYOUT[family]['lengths'] and n - 1 - locs[-1] == LAYOUT[family]['tail']


def key_strings(d):
    return np.array(['%s|%s|%s' % (k, v.dtype.name, ','.join(map(str, v.shape))) for k, v in d.items()])


def ingest_block(utils, out, tmp):
    rng = np.random.RandomState(20261)
    for family in ('ant', 'visual', 'powder', 'one'):
        raw = raw_columns(family, rng)
        check_layout(family, raw['terminals'])
        path = os.path.join(tmp, family + '.npz')
        np.savez(path, **raw)
        for k, v in raw.items():
            out[f'raw_{family}_{k}'] = v
        for compact in (True, False):
            mode = 'compact' if compact else 'regular'
            loads = {}
            for info in (True, False):
                d = utils.load_dataset(path, compact_dataset=compact, add_info=info, **LOAD_KW[family])
                d = {k: np.asarray(v) for k, v in d.items()}
                loads[info] = d
                out[f'keys_{family}_{mode}_{"info" if info else "noinfo"}'] = key_strings(d)
            full, lean = loads[True], loads[False]
            assert [k for k in full if k not in ('qpos', 'qvel', 'button_states')] == list(lean)
            for k, v in lean.items():
                assert v.dtype == full[k].dtype and np.array_equal(v, full[k]), (family, mode, k)
            for k, v in full.items():
                same = k in raw and v.dtype == raw[k].dtype and v.shape == raw[k].shape and np.array_equal(v, raw[k])
                if compact and family != 'one':           # one: min(1 + 1, 1) is the raw terminal again
                    assert same ==(k not in ('terminals', 'valids')), (family, k)
                if not same:
                    out[f'exp_{family}_{mode}_{k}'] = v
            if not compact:
                n_ob, n_next = len(full['observations']), len(full['next_observations'])
                if family == 'visual':
                    # the file's last row is not terminal: the reference keeps it as an
                    # observation but has no next row for it.  Reference behaviour.
                    assert n_ob == n_next + 1, (n_ob, n_next)
                else:
                    assert n_ob == n_next
                if family == 'one':
                    assert n_ob == 0 and full['observations'].shape == (0, 29)


class _Unwrapped:
    _reward_task_id = 1
    _goal_tol = 1.0
    cur_goal_xy = None


class _Env:
    def __init__(self, goal, tol):
        self.unwrapped = _Unwrapped()
        self.unwrapped.cur_goal_xy = np.asarray(goal)
        self.unwrapped._goal_tol = tol

    def reset(self):
        return None


def reference_success(relabel, qpos, goal, tol):
    """relabel_dataset of the reference -> success as uint8 (rewards and masks
    checked to be its two restatements)."""
    ds = dict(qpos=qpos)
    relabel.relabel_dataset('antmaze-large-navigate-singletask-task1-v0', _Env(goal, tol), ds)
    r, m = ds['rewards'], ds['masks']
    assert r.dtype == np.float32 and m.dtype == np.float32
    s = r + 1.0
    assert set(np.unique(s)) <= {0.0, 1.0} and np.array_equal(m, 1.0 - s)
    return s.astype(np.uint8)


def _fma(a, b, c):
    """Correctly rounded a*b + c (one rounding), through exact rationals."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def relabel_block(relabel, out):
    rng = np.random.RandomState(20262)
    out['rb_goal'] = RB_GOAL
    gx, gy = (float(v) for v in RB_GOAL)
    for dt, dtype in (('f32', np.float32), ('f64', np.float64)):
        q = (RB_GOAL + rng.uniform(-1.5, 1.5, (RB_ROWS, 2))).astype(dtype)
        q64 = q.astype(np.float64)                           # NumPy upcasts f32 qpos against the f64 goal
        dx, dy = q64[:, 0] - gx, q64[:, 1] - gy
        plain = np.sqrt(dx * dx + dy * dy)
        assert np.array_equal(plain, np.linalg.norm(q[:, :2] - RB_GOAL, axis=-1))
        cx = np.array([math.sqrt(_fma(a, a, b * b)) for a, b in zip(dx.tolist(), dy.tolist())])
        cy = np.array([math.sqrt(_fma(b, b, a * a)) for a, b in zip(dx.tolist(), dy.tolist())])
        lo_c, hi_c = np.minimum(cx, cy), np.maximum(cx, cy)
        order = np.argsort(plain)
        inner = order[8:-8]                                  # never the extreme rows: both outcomes stay present
        # rows where both contracted forms move the same way come first
        smaller = [i for i in inner if plain[i] < lo_c[i]] + [i for i in inner if lo_c[i] == plain[i] < hi_c[i]]
        larger = [i for i in inner if hi_c[i] < plain[i]] + [i for i in inner if lo_c[i] < plain[i] == hi_c[i]]
        assert len(smaller) >= RB_K // 2 and len(larger) >= RB_K // 2, (len(smaller), len(larger))
        rows = np.array(smaller[: RB_K // 2] + larger[: RB_K // 2], np.int64)
        tol = plain[rows]
        succ = np.stack([reference_success(relabel, q, RB_GOAL, float(t)) for t in tol])
        below_rows = rows[RB_K // 2:]
        tol_below = np.where(hi_c[below_rows] < plain[below_rows], hi_c[below_rows], lo_c[below_rows])
        succ_below = np.stack([reference_success(relabel, q, RB_GOAL, float(t)) for t in tol_below])
        hits = {'x': 0, 'y': 0}
        for k, r in enumerate(rows):
            assert 0 < succ[k].sum() < RB_ROWS, 'both outcomes present'
            assert succ[k, r] == 1, 'row k sits on <= and is a success'
            if k < RB_K // 2:      # plain is the smaller: a contracted form fails row k
                assert plain[r] < hi_c[r] and (cx[r] > tol[k] or cy[r] > tol[k])
                hits['x'] += cx[r] > tol[k]
                hits['y'] += cy[r] > tol[k]
            else:                  # plain is the larger: contraction keeps row k at tol_k, adds it at tol_below
                j = k - RB_K // 2
                assert lo_c[r] < plain[r] and tol_below[j] < plain[r]
                assert 0 < succ_below[j].sum() < RB_ROWS and succ_below[j, r] == 0
                assert cx[r] <= tol_below[j] or cy[r] <= tol_below[j]
                hits['x'] += cx[r] <= tol_below[j]
                hits['y'] += cy[r] <= tol_below[j]
        # whichever operand a compiler folds into the fma, many rows notice
        assert hits['x'] >= RB_K // 2 and hits['y'] >= RB_K // 2, hits
        ds = dict(qpos=q)
        relabel.add_oracle_reps('antmaze-large-navigate-oraclerep-v0', _Env(RB_GOAL, 1.0), ds)
        assert ds['oracle_reps'].dtype == np.float32 and np.array_equal(ds['oracle_reps'], q.astype(np.float32))
        out[f'rb_{dt}_qpos'] = q
        out[f'rb_{dt}_rows'] = rows
        out[f'rb_{dt}_tol'] = tol
        out[f'rb_{dt}_succ'] = succ
        out[f'rb_{dt}_tol_below'] = tol_below
        out[f'rb_{dt}_succ_below'] = succ_below
        if dt == 'f64':
            out['rb_f64_reps'] = ds['oracle_reps']           # f32: equal to qpos itself (asserted above)
        print(f'relabel boundary {dt}: {len(smaller)} smaller / {len(larger)} larger candidates, hits {hits}')


def ant_relabel(relabel, out):
    q = out['raw_ant_qpos']
    s = reference_success(relabel, q, ANT_GOAL, ANT_TOL)
    assert 20 < s.sum() < len(s) - 20
    for n in (1, 257):                                        # per-row: a prefix's result is the prefix
        assert np.array_equal(reference_success(relabel, q[:n], ANT_GOAL, ANT_TOL), s[:n])
    ds = dict(qpos=q)
    relabel.add_oracle_reps('antmaze-large-navigate-oraclerep-v0', _Env(ANT_GOAL, ANT_TOL), ds)
    assert np.array_equal(ds['oracle_reps'], q[:, :2].astype(np.float32))
    out['ant_relabel_goal'] = ANT_GOAL
    out['ant_relabel_tol'] = np.float64(ANT_TOL)
    out['ant_relabel_succ'] = s


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give
    the same bytes on every run."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    utils, _, relabel = reference_modules()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ingest_block(utils, out, tmp)
    relabel_block(relabel, out)
    ant_relabel(relabel, out)
    path = os.path.join(HERE, 'ingest_golden.npz')
    save_deterministic(path, out)
    size = os.path.getsize(path)
    assert size <= 300_000, size
    print('ingest golden:', len(out), 'arrays,', size, 'bytes')


if __name__ == '__main__':
    main()
