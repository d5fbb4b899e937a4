"""CPU tests of hierarchical sampling over the episode ring: the wiring of
include/ogbx_online_hgc.h into the build and the Python layer, and the
restatement (tests/online_hgc_np.py: oracle/gcdataset_np.hgc_sample over the
snapshot of tests/online_np.OnlineNp) against the reference's recorded
behaviour (tests/golden/online_hgc_golden.npz, built by
tests/golden/make_golden_online_hgc.py)."""

import os
import re

import numpy as np
import pytest

import online_hgc_np as ohn
import online_np as onp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_hgc_golden.npz')
EXAMPLE = dict(observations=np.zeros(2), actions=np.zeros(2, np.float32), next_observations=np.zeros(2))
# high_value_subgoal_steps of the 4 x 64 golden samples, by regime (online_hgc_np.regimes)
REGIME_COUNTS = {
    'hiql': dict(full_step=86, clip_end=119, clip_goal=51, goal_behind=33, zero_steps=102, open_episode=131,
                 closed_episode=125, wrapped_subgoal=20),
    'hlow': dict(full_step=43, clip_end=115, clip_goal=98, goal_behind=29, zero_steps=120, open_episode=141,
                 closed_episode=115, wrapped_subgoal=23),
}


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def _same(got, exp, what=''):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, got.shape, exp.dtype, exp.shape)
    np.testing.assert_array_equal(got, exp, err_msg=what)


def _exports(header):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(ogbx_online_[a-z0-9_]+)\s*\(', text)))


def test_header_and_source_are_wired_into_the_build():
    mk = open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()
    assert 'online_hgc.hip' in mk and 'ogbx_online_hgc.h' in mk
    hdr = open(os.path.join(ROOT, 'include', 'ogbx_online_hgc.h')).read()
    assert re.search(r'#define\s+OGBX_ONLINE_HGC_API_VERSION\s+1\b', hdr)
    exports = _exports('ogbx_online_hgc.h')
    assert exports == ['ogbx_online_hgc_api_version', 'ogbx_online_hgc_sample']
    # the header it extends still declares exactly its own four
    assert _exports('ogbx_online.h') == ['ogbx_online_api_version', 'ogbx_online_clear', 'ogbx_online_gc_sample',
                                         'ogbx_online_insert']
    from ogbench_amd import _lib
    from ogbench_amd import datasets as D

    L = D._bind()
    assert L is _lib.lib()
    for fn in exports:
        assert hasattr(L, fn) and getattr(L, fn).argtypes is not None, fn
    assert L.ogbx_online_hgc_api_version() == 1
    import ogbench_amd

    assert 'HGCReplayBuffer' in ogbench_amd.__all__
    assert ogbench_amd.HGCReplayBuffer is D.HGCReplayBuffer and issubclass(D.HGCReplayBuffer, D.GCReplayBuffer)
    # every key a sample returns is refused as a column name
    assert set(D.GCReplayBuffer.RESERVED) < set(D.HGCReplayBuffer.RESERVED)
    assert {'high_value_reps', 'low_value_goals', 'high_actor_targets', 'low_actor_next_observations'} <= set(
        D.HGCReplayBuffer.RESERVED)


def _replay(gold, upto):
    ring = onp.OnlineNp(EXAMPLE, ohn.N, ohn.T)
    for t in range(upto):
        ring.add({k: gold[f'in_{k}'][t] for k in EXAMPLE}, gold['done'][t])
    return ring


def _draws(gold, pre):
    return {k[len(pre) + 5:]: v for k, v in gold.items() if k.startswith(pre + 'draw_')}


def test_golden_history_is_the_designed_one(gold):
    done = gold['done']
    assert done.shape == (ohn.STEPS, ohn.N) == (31, 5) and gold['snap_steps'].tolist() == list(ohn.SNAPS)
    for e, steps in ohn.DONE_AT.items():
        assert np.flatnonzero(done[:, e]).tolist() == list(steps)
    assert (~done.any(0)).any()  # an env that is never done
    assert (done[1:] & done[:-1]).any()  # an episode of length 1
    assert all(v.dtype != object and v.nbytes <= 4096 for v in gold.values())  # arrays only


@pytest.mark.parametrize('S', ohn.SNAPS)
def test_restatement_over_the_ring_reproduces_the_reference(gold, S):
    ring = _replay(gold, S)
    snap = ring.snapshot()
    assert sorted(snap) == sorted(k[len(f's{S}_snap_'):] for k in gold if k.startswith(f's{S}_snap_'))
    for k, v in snap.items():
        _same(v, gold[f's{S}_snap_{k}'], k)
    for cname, cfg in ohn.GOLDEN_CONFIGS.items():
        pre = f's{S}_{cname}_'
        out, ix = ohn.hgc_sample(ring, cfg, _draws(gold, pre))
        keys = gold[pre + 'keys'].tolist()
        assert len(keys) == dict(hiql=26, hlow=27, hcur=27)[cname]
        assert list(out) == [k for k in keys if k != 'terminals']  # the snapshot's own column
        for k, v in out.items():
            _same(v, gold[pre + 'out_' + k], f'{cname} {k}')
        assert ('low_value_goals' in out) == (cfg.get('low_discount') is not None)
        np.testing.assert_array_equal(ix['hvg'] - ix['idxs'], gold[pre + 'out_high_value_offsets'])


@pytest.mark.parametrize('cname', ['hiql', 'hlow'])
def test_golden_samples_reach_every_regime(gold, cname):
    """From the fixture alone: full steps, steps clipped by the episode end and
    by the goal, goals behind the sample, zero steps, open and closed episodes,
    and subgoal rows physically below their sample's (the ring wrapped)."""
    cfg = ohn.GOLDEN_CONFIGS[cname]
    seen = dict.fromkeys(ohn.REGIMES, 0)
    for S in ohn.SNAPS:
        ring = _replay(gold, S)
        pre = f's{S}_{cname}_'
        idxs = gold[pre + 'draw_pick']
        hvg = idxs + gold[pre + 'out_high_value_offsets']
        r = ohn.regimes(ring, idxs, hvg, gold[pre + 'out_high_value_subgoal_steps'], ohn.value_steps(cfg))
        for k, v in r.items():
            seen[k] += v
    assert all(v >= 1 for v in seen.values()), seen
    assert seen == REGIME_COUNTS[cname]


def test_hcur_covers_the_actor_side(gold):
    """value goal = current state: every value step is 0; the actor subgoals
    use high_subgoal_steps = 5."""
    cfg = ohn.GOLDEN_CONFIGS['hcur']
    assert ohn.value_steps(cfg) == 5
    moved = 0
    for S in ohn.SNAPS:
        pre = f's{S}_hcur_'
        assert not gold[pre + 'out_high_value_subgoal_steps'].any() and not gold[pre + 'out_high_value_offsets'].any()
        moved += int((gold[pre + 'out_high_actor_next_observations'] != gold[pre + 'out_observations']).any(1).sum())
    assert moved >= 1
