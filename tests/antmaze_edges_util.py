"""Shared helpers of tests/test_antmaze_cpu.py and tests/test_antmaze_edges_gpu.py
for tests/golden/antmaze_edges_golden.npz (make_golden_ant_edges.py): block
access, the oracle run of a block, bit-for-bit comparison, and a NumPy
restatement of antmaze.h's Philox body draws."""

import json
import os

import numpy as np

from oracle import antmaze_np as am
from oracle import locomaze as orc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EDGES = os.path.join(GOLDEN_DIR, 'antmaze_edges_golden.npz')
BLOCKS = ('cfg1', 'cfg2', 'edge', 'tp', 'ep')
TIMINGS = ('post', 'pre')
N = 70
EDGE_PLAIN, EDGE_A, EDGE_B, EDGE_C = 0, 1, 2, 3
# constructor options of each block (the rest are the defaults)
CONFIG = {
    'cfg1': dict(terminate_at_goal=False, add_noise_to_goal=True),
    'cfg2': dict(terminate_at_goal=True, reward_task_id=3, add_noise_to_goal=False),
    'edge': {}, 'tp': {}, 'ep': {},
}
MAZE = {'cfg1': 'large', 'cfg2': 'large', 'edge': 'large', 'tp': 'teleport', 'ep': 'large'}
TAG_TELEPORT = 0x4D5A0002
TAG_ANT_BODY = 0x414E0001

_cache = {}


def load():
    if 'd' not in _cache:
        _cache['d'] = dict(np.load(EDGES))
    return _cache['d']


def block(name, timing):
    p = f'{name}_{timing}_'
    return {k[len(p):]: v for k, v in load().items() if k.startswith(p)}


def teleport_info():
    return json.load(open(os.path.join(GOLDEN_DIR, 'teleport_golden.json')))


def same_bits(a, b):
    """Bit-for-bit equality (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


def oracle_batch(name, timing, g):
    kw = dict(CONFIG[name])
    tasks = am.LARGE_TASKS
    if name == 'tp':
        kw.update(teleport=am.teleport_table(teleport_info()), task_xy=g['task_xy'])
        tasks = am.TELEPORT_TASKS
    return am.Batch(np.maximum(g['task'], 1), g['noise'], g['body_draws'], max_steps=int(g['max_steps']),
                    timing=timing, tasks=tasks, track_body=True, **kw)


def oracle_step(name, b, g, t):
    kw = {}
    if name == 'tp':
        kw['tp_out'] = g['tp_draws'][t]
    if name == 'ep':
        kw.update(reset_noise=g['reset_noise'][t], reset_states=g['reset_states'][t])
    return b.step(g['qpos_post'][t], g['qvel_post'][t], auto_reset=name == 'ep', **kw)


def teleport_index(seed, gi, episode, elapsed, n_out=3):
    """The out-portal index libogbx draws for global env gi at that step
    (antmaze.h phase A; tests/test_antmaze_gpu.py::test_teleport_moves_body_xy)."""
    k0, k1 = orc.philox_key(seed, orc.TAG_MAZE_RESET)
    w = orc.philox4x32([gi & 0xFFFFFFFF, episode, 0x100 + elapsed, gi >> 32], k0 ^ TAG_TELEPORT, k1)
    return (int(w[0]) * n_out) >> 32


def u01_from(hi, lo):
    """common.h u01_from: the top 53 bits of (hi, lo) as a double in [0, 1)."""
    return float(((int(hi) << 32 | int(lo)) >> 11)) * 2.0 ** -53


def body_uniforms(seed, gi, episode, slot):
    """The Philox uniforms behind ant_body_draw(gi, episode, c, ..., slot) for
    c = 0..28: (u0, u1) [29, 2]; counter (gi lo, episode, slot + c, gi hi),
    key (k0 ^ kTagAntBody, k1) of the handle's reset key."""
    k0, k1 = orc.philox_key(seed, orc.TAG_MAZE_RESET)
    out = np.zeros((29, 2))
    for c in range(29):
        w = orc.philox4x32([gi & 0xFFFFFFFF, episode, slot + c, gi >> 32], k0 ^ TAG_ANT_BODY, k1)
        out[c] = u01_from(w[0], w[1]), u01_from(w[2], w[3])
    return out


def body_state_from_uniforms(u):
    """The reset_model state antmaze.h builds from body_uniforms: qpos0 +
    (-0.1 + 0.2 u0) for the 15 positions (exact double arithmetic), and
    0.1 * sqrt(-2 log1p(-u0)) cospi(2 u1) (Box-Muller) for the 14 velocities in
    np.longdouble.  Returns (qpos [15] float64, qvel [14] longdouble)."""
    q = am.QPOS0 + (-0.1 + 0.2 * u[:15, 0])
    ld = np.longdouble
    u0, u1 = u[15:, 0].astype(ld), u[15:, 1].astype(ld)
    r = np.sqrt(ld(-2) * np.log1p(-u0))
    # cospi(2 u1) with the argument reduced exactly first: 2 u1 = k + f, k the nearest multiple of 1/2
    # and |f| <= 1/4, then cos / sin of pi f (pi rounded once, in long double)
    two = ld(2) * u1
    k = np.round(two * 2) / 2
    f = (two - k) * ld('3.14159265358979323846264338327950288')
    quad = np.round(k * 2).astype(np.int64) % 4
    c = np.where(quad == 0, np.cos(f), np.where(quad == 1, -np.sin(f), np.where(quad == 2, -np.cos(f), np.sin(f))))
    return q, ld(0.1) * (r * c)


def ulp_distance(got, ref_ld):
    """|got - ref| in units of the double ulp at ref (ref in long double)."""
    ref = np.asarray(ref_ld, np.longdouble)
    ulp = np.spacing(np.abs(ref.astype(np.float64)))
    return np.abs(np.asarray(got, np.longdouble) - ref) / ulp
