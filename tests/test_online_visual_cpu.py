"""CPU checks of visual batches over the episode ring and of the
ogbx_online_visual.h boundary: the NumPy restatement
(tests/online_visual_np.py) reproduces every array put together from the
reference's own code (tests/golden/online_visual_golden.npz, built by
tests/golden/make_golden_online_visual.py), its two forms of the stack agree on
random histories, libogbx.so exports every symbol of the header, and the
argument checks run before any device call."""

import ctypes
import os
import re

import numpy as np
import pytest

import online_np as onp
import online_visual_np as ovn
from ogbench_amd import _lib, _online_visual
from ogbench_amd import datasets as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_visual_golden.npz')
HEADER = os.path.join(ROOT, 'include', 'ogbx_online_visual.h')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _replay(gold, upto):
    ring = onp.OnlineNp(ovn.EXAMPLE, ovn.N, ovn.T)
    for t in range(upto):
        ring.add({k: gold[f'in_{k}'][t] for k in ovn.EXAMPLE}, gold['done'][t])
    return ring


def case(gold, S, cname):
    """(draws without crop_from, crop_from, expected batch without the
    snapshot's terminals, in the reference's key order)."""
    pre = f's{S}_{cname}_'
    draws = {k[len(pre) + 5:]: v for k, v in gold.items() if k.startswith(pre + 'draw_')}
    crop_from = draws.pop('crop_from')
    keys = [k for k in gold[pre + 'keys'].tolist() if k != 'terminals']
    return draws, crop_from, {k: gold[pre + 'out_' + k] for k in keys}


# ------------------------------------------------------------------- the fixture
def test_fixture_history_is_the_designed_one(gold):
    rows, done = ovn.history()
    assert gold['snap_steps'].tolist() == list(ovn.SNAPS) and np.array_equal(gold['done'], done)
    for k, v in rows.items():
        assert gold[f'in_{k}'].dtype == v.dtype and np.array_equal(gold[f'in_{k}'], v), k
    obs, nxt = rows['observations'], rows['next_observations']
    assert obs.shape == (17, 5, 6, 5, 2) and obs.dtype == np.uint8
    for t in range(16):  # next_observations[t] == observations[t + 1] inside an episode, and only there
        for e in range(5):
            assert np.array_equal(nxt[t, e], obs[t + 1, e]) == (not done[t, e]), (t, e)
    frames = {obs[t, e].tobytes() for t in range(17) for e in range(5)}
    assert len(frames) == 17 * 5  # the pixels tell every (env, step) apart
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'visual_golden.npz'))
    assert all(v.dtype != object for v in gold.values())


@pytest.mark.parametrize('cname', list(ovn.GOLDEN_CONFIGS))
@pytest.mark.parametrize('S', ovn.SNAPS)
def test_restatement_reproduces_the_fixture(gold, S, cname):
    cfg, hgc = ovn.GOLDEN_CONFIGS[cname], ovn.HGC[cname]
    draws, crop_from, exp = case(gold, S, cname)
    out, ix = ovn.sample(_replay(gold, S), cfg, draws, crop_from, hgc=hgc)
    assert list(out) == list(exp)
    for k, v in exp.items():
        assert out[k].dtype == v.dtype and out[k].shape == v.shape, (k, out[k].dtype, out[k].shape, v.shape)
        np.testing.assert_array_equal(out[k], v, err_msg=k)
    assert out['observations'].shape == (ovn.B, 6, 5, 2 * ovn.F_GOLD)
    assert crop_from.shape == (ovn.B, 2) and crop_from.min() >= 0 and crop_from.max() <= 2 * ovn.PADDING


def test_fixture_holds_the_designed_cases(gold):
    """From the ring's tables alone: stacks cut by 1 and 2 frames at an episode
    start and at the oldest live row, a stack whose physical rows wrap, an
    episode of length 1, a clamped goal stack, and the crop's corners."""
    seen = dict(cut_at_start=set(), cut_at_oldest=set(), wraps=0, length_one=0, goal_cut=0)
    offs = [set(), set()]
    done = gold['done']
    for S in ovn.SNAPS:
        ring = _replay(gold, S)
        first = S - ring.L
        for cname, cfg in ovn.GOLDEN_CONFIGS.items():
            draws, crop_from, _ = case(gold, S, cname)
            _, ix = ovn.sample(ring, cfg, draws, crop_from, hgc=ovn.HGC[cname])
            idxs, goal = ix['idxs'], ix['hvg' if ovn.HGC[cname] else 'vg']
            src = ovn.stack_flat(ring, idxs, ovn.F_GOLD)
            e, k = ring.split(idxs)
            for b in range(len(idxs)):
                depth = len(set(src[b].tolist()))
                t, t0 = first + k[b], first + ring.split(src[b, 0])[1]  # the row's step, its stack's first
                if depth < ovn.F_GOLD:
                    started = t0 == 0 or done[t0 - 1, e[b]]  # else the episode's head was overwritten
                    assert started or t0 == first
                    (seen['cut_at_start'] if started else seen['cut_at_oldest']).add(depth)
                seen['wraps'] += int((np.diff(ring.phys(src[b])) < 0).any())
                seen['length_one'] += int(done[t, e[b]] and (t == 0 or done[t - 1, e[b]]))
            gsrc = ovn.stack_flat(ring, goal[goal != idxs], ovn.F_GOLD)
            seen['goal_cut'] += int(sum(len(set(r)) < ovn.F_GOLD for r in gsrc.tolist()))
            for ax in range(2):
                offs[ax] |= set(crop_from[:, ax].tolist())
    assert seen['cut_at_start'] == {1, 2} and seen['cut_at_oldest'] >= {1, 2}, seen
    assert seen['wraps'] >= 1 and seen['length_one'] >= 1 and seen['goal_cut'] >= 1, seen
    assert offs[0] == offs[1] == set(range(7))


# ---------------------------------------------------------- the stack's two forms
@pytest.mark.parametrize('p', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('N,T', [(1, 1), (1, 3), (3, 2), (5, 6)])
def test_the_table_form_equals_the_snapshot_form(N, T, p):
    """ep_seq with the liveness bound against get_stacked_observations' rule
    over the snapshot, for every live row after every step; p = 0 is the env
    that is never done, whose dead slots hold rows of an equal ep_seq."""
    rng = np.random.RandomState(100 * N + 10 * T + int(10 * p))
    ex = dict(observations=np.zeros(2), next_observations=np.zeros(2))
    ring = onp.OnlineNp(ex, N, T)
    for step in range(3 * T + 2):
        ring.add(dict(observations=rng.normal(size=(N, 2)), next_observations=rng.normal(size=(N, 2))),
                 rng.rand(N) < p)
        flat = np.arange(N * ring.L)
        for F in (1, 2, 3, 8):
            a, b = ovn.stack_flat(ring, flat, F), ovn.stack_flat_snapshot(ring, flat, F)
            np.testing.assert_array_equal(a, b, err_msg=f'step {step} F {F}')
            assert (a[:, -1] == flat).all() and (np.diff(a, axis=1) >= 0).all()
            assert (a // ring.L == (flat // ring.L)[:, None]).all()  # a stack never leaves its env
        if p == 0.0 and ring.S > T:  # the oldest live row of a never-done env: a stack of one frame
            assert (ovn.stack_flat(ring, np.arange(N) * ring.L, 8) == (np.arange(N) * ring.L)[:, None]).all()


# ------------------------------------------------------------------- the boundary
def header_symbols():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(ogbx_online_visual_[a-z0-9_]+)\s*\(', text)))


def test_symbols_exported_bound_and_versioned():
    L = _online_visual.bind()
    assert L is _lib.lib()
    syms = header_symbols()
    assert syms == ['ogbx_online_visual_api_version', 'ogbx_online_visual_gather']
    for s in syms:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
    want = int(re.search(r'#define\s+OGBX_ONLINE_VISUAL_API_VERSION\s+(\d+)', open(HEADER).read()).group(1))
    assert L.ogbx_online_visual_api_version() == want == _online_visual.ONLINE_VISUAL_API_VERSION == 1
    # an extension: ogbx.h's ABI and the other extensions' versions are as they were
    assert not set(syms) & set(_lib.declared_symbols())
    D._bind()
    assert (L.ogbx_abi_version(), L.ogbx_visual_api_version(), L.ogbx_online_api_version(),
            L.ogbx_online_hgc_api_version()) == (5, 1, 1, 1)


def test_header_and_source_are_wired_into_the_build_and_documented():
    mk = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert 'online_visual.hip' in mk and 'ogbx_online_visual.h' in mk
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'ogbx_online_visual.h' in doc and [s for s in header_symbols() if s not in doc] == []
    src = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'online_visual.hip')).read()
    assert '__global__' in src and 'online_visual_gather_kernel' in src


def test_argument_checks_precede_device_calls():
    """NULL pointers, the ring's ranges, an empty ring, total, the column
    count, frame_stack, padding, the selectors (1 and HGC's without hcfg), a
    missing index output and a non-positive geometry are refused (OGBX_EINVAL,
    message in ogbx_last_error) on any host: no pointer is dereferenced."""
    L = _online_visual.bind()
    Col = _online_visual.OnlineVisualColumn

    def ring(n=4, t=3, s=5, a=8, b=8, c=8):
        return D.OnlineRing(n, t, s, a, b, c)

    idx = D.VisualIndices(8, None, None, None)
    hidx = D.VisualIndices(8, 8, 8, None)
    hcfg = D.HgcConfig(2, 2, 2, 0, 0, 0.0, 8, 8, 8, 8)

    def col(src=8, alt=None, dst=8, h=4, w=4, px=3, select=0, stack=1, crop=1):
        return Col(src, alt, dst, h, w, px, select, stack, crop)

    def call(cols=(col(),), r='ring', i=idx, h=None, ncols=None, total=4, F=3, pad=3, crop_out=None):
        arr = (Col * max(1, len(cols)))(*cols) if cols is not None else None
        st = L.ogbx_online_visual_gather(ring() if r == 'ring' else r, h, arr, len(cols) if ncols is None else ncols,
                                         total, i, F, pad, None, 0, 0, 0, crop_out, None)
        return st, _lib.last_error()

    bad = dict(
        null_ring=dict(r=None), null_indices=dict(i=None), null_cols=dict(cols=None, ncols=1),
        null_idxs=dict(i=D.VisualIndices(None, None, None, None)),
        null_ep_seq=dict(r=ring(a=None)), null_cur_seq=dict(r=ring(b=None)), null_ep_end=dict(r=ring(c=None)),
        n_zero=dict(r=ring(n=0)), t_zero=dict(r=ring(t=0)), n_huge=dict(r=ring(n=1 << 31)),
        rows_huge=dict(r=ring(n=(1 << 31) - 1, t=(1 << 31) - 1)), steps_negative=dict(r=ring(s=-1)),
        empty_ring=dict(r=ring(s=0)), total_zero=dict(total=0), total_negative=dict(total=-3),
        no_columns=dict(cols=(), ncols=0), too_many_columns=dict(cols=(col(),) * 17),
        frame_stack_zero=dict(F=0), frame_stack_nine=dict(F=9), padding_negative=dict(pad=-1),
        select_next=dict(cols=(col(select=1),)), select_hgc_without_hcfg=dict(cols=(col(select=4),), i=hidx),
        select_ten=dict(cols=(col(select=10),), i=hidx, h=hcfg), select_negative=dict(cols=(col(select=-1),)),
        select_next_hgc=dict(cols=(col(select=1),), i=hidx, h=hcfg),
        missing_value_goals=dict(cols=(col(select=2),)), missing_actor_goals=dict(cols=(col(select=3),)),
        missing_low_goals=dict(cols=(col(select=6),), i=hidx, h=hcfg),
        null_src=dict(cols=(col(src=None),)), null_dst=dict(cols=(col(dst=None),)),
        height_zero=dict(cols=(col(h=0),)), width_negative=dict(cols=(col(w=-2),)), px_zero=dict(cols=(col(px=0),)),
        crop_out_without_offsets=dict(crop_out=8),
        negative_subgoal_steps=dict(h=D.HgcConfig(2, -1, 2, 0, 0, 0.0, 8, 8, 8, 8), i=hidx),
    )
    for name, kw in bad.items():
        st, msg = call(**kw)
        assert st == _lib.OGBX_EINVAL, name
        assert msg.startswith('ogbx_online_visual_gather: '), (name, msg)
    for name, word in (('frame_stack_nine', 'frame_stack'), ('padding_negative', 'padding'),
                       ('select_next', 'selector'), ('missing_value_goals', 'missing index'),
                       ('empty_ring', 'empty'), ('total_zero', 'total'), ('too_many_columns', 'columns'),
                       ('height_zero', 'image shape')):
        assert word in call(**bad[name])[1], name
