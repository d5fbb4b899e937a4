"""CPU checks of the fused point-maze collector's host side: the exports of
include/ogbx_collect.h, stitch_cells against a literal transcription of
generate_locomaze.py's BFS (tests/collect_np.py), and collect_locomaze's
argument checks."""

import os
import re

import numpy as np
import pytest

import collect_np
from ogbench_amd import _lib
from ogbench_amd.datagen import collect_locomaze, maze_cells, stitch_cells
from ogbench_amd.locomaze import static_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAZES = ('arena', 'medium', 'large', 'giant', 'teleport')


def test_library_exports_the_collect_header():
    from ogbench_amd import _collect

    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ogbx_collect.h')).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(ogbx_[a-z0-9_]+)\s*\(', text)))
    assert declared == ['ogbx_collect_abi_version', 'ogbx_maze_collect']
    L = _collect.bind()
    assert [s for s in declared if not hasattr(L, s)] == []
    assert L.ogbx_collect_abi_version() == 1
    assert int(re.search(r'#define\s+OGBX_COLLECT_ABI_VERSION\s+(\d+)', text).group(1)) == 1
    # ogbx.h's own version is untouched by the extension
    assert L.ogbx_abi_version() == 5
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert [s for s in declared if s not in doc] == []
    # the Makefile rebuilds the library when the header changes
    assert 'ogbx_collect.h' in open(os.path.join(ROOT, 'ogbench_amd', 'csrc', 'Makefile')).read()


def test_collect_structs_match_the_header_layout():
    import ctypes

    from ogbench_amd import _collect

    assert ctypes.sizeof(_collect.CollectConfig) == 32 and _collect.CollectConfig.goal_cells.offset == 16
    assert ctypes.sizeof(_collect.CollectTape) == 40 and _collect.CollectTape.steps.offset == 32
    assert ctypes.sizeof(_collect.CollectOutputs) == 72 and _collect.CollectOutputs.row_stride.offset == 32


@pytest.mark.parametrize('maze', MAZES)
def test_stitch_cells_equal_the_script_bfs(maze):
    mp, _ = static_tables(maze)
    all_cells, _ = maze_cells(mp)
    adj, count = stitch_cells(mp)
    assert adj.dtype == np.int32 and count.dtype == np.int32
    assert adj.shape[0] == count.shape[0] == len(all_cells) and adj.shape[2] == 2
    for c, ij in enumerate(all_cells):
        ij = (int(ij[0]), int(ij[1]))
        want = collect_np.script_adj_cells(mp, ij)
        got = [tuple(int(v) for v in row) for row in adj[c, :count[c]]]
        assert got == want, (maze, ij)
        assert (adj[c, count[c]:] == -1).all()
        dist = collect_np.bfs_distances(mp, ij)
        for cell in got:
            assert mp[cell] == 0 and dist[cell] == 4
        # and no cell at distance 4 is left out
        assert len(got) == int((dist == 4).sum())
    assert count.max() <= 8
    if maze != 'arena':
        assert count.max() <= 6
    assert int((count == 0).sum()) == (1 if maze == 'teleport' else 0)


def test_stitch_cells_arena_maximum_is_8():
    assert stitch_cells(static_tables('arena')[0])[1].max() == 8


def test_stitch_cells_small_open_map_has_no_candidates():
    """Maps on which no cell is 4 steps from any other: every list is empty (the
    script's goal = init fallback) and the table keeps one padded column."""
    mp = np.ones((3, 3), np.int32)
    mp[1, 1] = 0  # a 3x3 map: one open cell inside its border
    adj, count = stitch_cells(mp)
    assert count.tolist() == [0] and adj.shape == (1, 1, 2) and (adj == -1).all()
    mp = np.ones((4, 5), np.int32)
    mp[1:3, 1:4] = 0  # a 2x3 room: the farthest pair is 3 steps apart
    adj, count = stitch_cells(mp)
    assert count.tolist() == [0] * 6 and adj.shape == (6, 1, 2) and (adj == -1).all()
    mp = np.ones((5, 5), np.int32)
    mp[1:4, 1:4] = 0  # a 3x3 room has nothing 5 steps away
    adj, count = stitch_cells(mp, adj_steps=5)
    assert count.tolist() == [0] * 9 and (adj == -1).all()


def test_stitch_cells_3x3_open_map():
    """3x3 open room: the only pairs 4 steps apart are opposite corners."""
    mp = np.ones((5, 5), np.int32)
    mp[1:4, 1:4] = 0
    adj, count = stitch_cells(mp)
    all_cells, _ = maze_cells(mp)
    for c, (i, j) in enumerate(all_cells):
        want = collect_np.script_adj_cells(mp, (int(i), int(j)))
        assert [tuple(r) for r in adj[c, :count[c]].tolist()] == want
        assert count[c] == (1 if (i in (1, 3) and j in (1, 3)) else 0)


def test_stitch_cells_is_pure():
    mp, _ = static_tables('medium')
    before = mp.copy()
    a1, c1 = stitch_cells(mp)
    a2, c2 = stitch_cells(mp)
    assert np.array_equal(mp, before) and np.array_equal(a1, a2) and np.array_equal(c1, c2)


@pytest.mark.parametrize('kw, match', [
    (dict(dataset_type='wander'), 'dataset_type'),
    (dict(dataset_type='stitch', fused=False), 'fused'),
    (dict(dataset_type='explore', fused=False), 'fused'),
    (dict(num_envs=0), 'num_envs'),
    (dict(num_rounds=-1), 'num_rounds'),
    (dict(max_episode_steps=0), 'max_episode_steps'),
    (dict(chunk=0, fused=True), 'chunk'),
    (dict(chunk=2.5, fused=True), 'chunk'),
    (dict(noise=-0.1), 'noise'),
    (dict(noise=float('nan')), 'noise'),
    (dict(fused='yes'), 'fused'),
    (dict(tape=dict(normal=np.zeros((1, 25, 4, 2))), num_envs=4, max_episode_steps=25), 'fused path only'),
    (dict(tape=dict(normal=np.zeros((1, 25, 3, 2))), fused=True, num_envs=4, max_episode_steps=25), 'shape'),
    (dict(tape=dict(normal=np.zeros((2, 25, 4, 2))), fused=True, num_envs=4, max_episode_steps=25), 'num_rounds'),
    (dict(tape=dict(normal=np.zeros((1, 20, 4, 2))), fused=True, num_envs=4, max_episode_steps=25), 'covers'),
    (dict(tape=dict(dir=np.zeros((1, 2, 4, 2)), normal=np.zeros((1, 25, 4, 2))), fused=True, num_envs=4,
          max_episode_steps=25), 'shape'),
    (dict(tape=dict(wind=np.zeros((1, 25, 4, 2))), fused=True, num_envs=4, max_episode_steps=25), 'keys'),
])
def test_collect_locomaze_refuses_bad_arguments_before_any_device(kw, match, monkeypatch):
    import ogbench_amd.registry as registry

    def no_device(*a, **k):
        raise AssertionError('an env was made before the arguments were checked')

    monkeypatch.setattr(registry, 'make', no_device)
    with pytest.raises(ValueError, match=match):
        collect_locomaze('pointmaze-medium-v0', **kw)
