"""CPU: the case matrix of tests/test_gather_gpu.py reaches every branch of the
samplers' row gather (copy_tile / copy_rows, csrc/gc_device.h) by construction,
and the restated tile numbering hands every sample to exactly one workgroup.
The branches cannot be observed from outside, so this is the proof that the GPU
sweep takes them: the rules of tests/gather_np.py applied to its own tables."""

import numpy as np

import gather_np as G


def test_unit_rule_on_the_ingest_table():
    """The copy-unit rule, on the table of test_ingest_gpu.py's docstring plus
    the stride column: a stride narrows exactly as a pointer does."""
    table = {
        (1, 3, 259): (1, 1, 1, 1, 1, 1, 1),
        (4, 12, 116, 20, 260, 276, 508, 516): (4, 4, 4, 1, 4, 4, 1),
        (8, 24, 232, 520, 1608): (8, 8, 4, 1, 4, 8, 1),
        (16, 48, 256, 512, 528, 12288): (16, 8, 4, 1, 4, 8, 1),
    }
    assert sorted(rb for rbs in table for rb in rbs) == sorted(G.ROW_BYTES)
    for rbs, widths in table.items():
        for rb in rbs:
            for (so, do), w in zip(G.OFFSETS, widths):
                assert G.copy_unit(rb, so, do, 0) == w, (rb, so, do)
                assert G.copy_unit(rb, so, do, rb) == w
    assert G.copy_unit(48, 0, 0, 48 + 4) == 4 and G.copy_unit(48, 0, 0, 48 + 8) == 8
    assert G.copy_unit(48, 0, 0, 48 + 16) == 16 and G.copy_unit(12, 8, 0, 32) == 4


def test_matrix_reaches_every_unit_class_path_and_wave():
    """Every (unit, units per row, flat, wave0) that exists is reached."""
    reached = set()
    narrowed_by = set()
    for entry in G.ENTRY_TABLE:
        size, nsel = G.ENTRY_TABLE[entry]
        for rb in G.ROW_BYTES:
            assert rb == 12 or len(G.sweep_combos(rb)) == len(G.OFFSETS) * len(G.STRIDE_PADS)
            seen = set()
            for t in G.sweep_tables(rb, entry):
                assert 1 <= len(t) <= size and all(0 <= c['select'] < nsel for c in t)
                assert all(c['stride'] == 0 or c['stride'] >= rb for c in t)
                seen |= {(c['src_off'], c['dst_off'], c['stride']) for c in t}
                for total in G.SWEEP_TOTALS:
                    reached |= G.reach(t, G.flat4_tiled(t, total), 0)
                for c in t:     # a unit below the row's own, through exactly one of the three
                    full = G.copy_unit(rb, 0, 0, 0)
                    alone = {'src': G.copy_unit(rb, c['src_off'], 0, 0), 'dst': G.copy_unit(rb, 0, c['dst_off'], 0),
                             'stride': G.copy_unit(rb, 0, 0, c['stride'])}
                    narrow = [k for k, w in alone.items() if w < full]
                    if len(narrow) == 1:
                        assert G.spec_unit(c) == alone[narrow[0]] < full
                        narrowed_by.add(narrow[0])
            assert seen >= set(G.sweep_combos(rb)), rb     # no combination lost in the chunking
    assert narrowed_by == {'src', 'dst', 'stride'}
    for nsel in (4, 10):
        for form, wave0 in G.AHEAD_FORMS.items():
            t = G.ahead_nonflat_table(nsel)
            assert not G.flat4_table(t) and len(t) <= 16
            reached |= G.reach(t, False, wave0)
            for n in G.AHEAD_FLAT_COLS:
                reached |= G.reach(G.flat_table(n, nsel), True, wave0)
    missing = G.feasible_reach() - reached
    assert not missing, sorted(missing)
    # the packed record: a 12-byte column at offset 8 of a 32-byte record
    assert (8, 0, 32) in G.sweep_combos(12) and G.copy_unit(12, 8, 0, 32) == 4


def test_flat_rule_edges():
    """512 B is flat and 516 B is not; one 1-byte column makes a flat table
    non-flat; the tiled kernels leave the job path at 5120 samples."""
    assert G.flat4_table([G.col(512)]) and not G.flat4_table([G.col(516)])
    assert G.flat4_table([G.col(508, 4, 8, 512)]) and not G.flat4_table([G.col(508, 4, 8, 510)])
    for total in G.EDGE_TOTALS:
        t = G.edge_tables(total)
        assert G.flat4_table(t['flat']) and not G.flat4_table(t['byte'])
        assert G.flat4_table(t['byte'][:-1]) and t['byte'][-1]['row_bytes'] == 1
        assert G.flat4_tiled(t['flat'], total) == (total < 5120)
        assert not G.flat4_tiled(t['byte'], total)
        assert total < G.EDGE_LARGE or all(len(x) <= 3 and max(c['row_bytes'] for c in x) <= 20 for x in t.values())
    carry = set()     # rows of more units than threads in a tile of several samples: every unit
    for total in G.EDGE_TOTALS:
        wide = G.edge_tables(total).get('wide', [])
        assert not G.flat4_table(wide) or not wide
        if G.gc_tile(total) > 1:
            carry |= {(G.spec_unit(c), G.units_class(c['row_bytes'] // G.spec_unit(c))) for c in wide}
    assert carry >= {(w, 'above256') for w in (16, 8, 4, 1)} | {(4, 'between'), (4, 'several'), (1, 'several')}
    assert G.gc_tile(5119) == 4 and G.gc_tile(5120) == 5 and G.gc_tile(65536) == 64 == G.gc_tile(1 << 30)
    assert [G.gc_tile(t) for t in (1, 1023, 1024, 2047, 2048, 4099)] == [1, 1, 1, 1, 2, 4]
    assert not G.flat4_table(G.hgc_table(False)) and G.flat4_table(G.hgc_table(True))
    assert {c['select'] for c in G.hgc_table(True)} == set(range(10))
    for rb in G.ROW_BYTES:     # the sweep's flat tables are exactly the rows the job path takes
        for entry in G.ENTRY_TABLE:
            flat = [t for t in G.sweep_tables(rb, entry) if G.flat4_table(t)]
            assert bool(flat) == (rb % 4 == 0 and rb <= 512), rb
    two_slots = {rb for rb in G.ROW_BYTES if rb % 4 == 0 and 256 < rb <= 512}
    assert {260, 508, 512} <= two_slots and 256 in G.ROW_BYTES and 516 in G.ROW_BYTES


def test_job_loop_trips():
    """num_cols x n_here of 24, 25, 32, 33, 36 and 128; one trip, exactly one
    full trip and more than one, with four copying waves and with three; table
    sizes 1, 9, 16, 17 and 32 at tiles 1 and 4."""
    counts, trips4, sizes = set(), set(), set()
    for n, total in G.JOB_CASES:
        assert G.flat4_tiled(G.flat_table(n, 4), total)
        for jobs in G.job_counts(n, total):
            counts.add(jobs)
            trips4.add(G.job_trips(jobs, 4))
        sizes.add((n, G.gc_tile(total)))
    assert {24, 25, 32, 33, 36, 128} <= counts
    assert trips4 == {'part', 'full', 'many'}
    assert {(n, t) for n in (1, 9, 16, 17, 32) for t in (1, 4)} <= sizes
    assert G.job_trips(32, 4) == 'full' and G.job_trips(24, 3) == 'full'
    trips3 = {G.job_trips(n, 3) for n in G.AHEAD_FLAT_COLS}      # look-ahead: tile 1, jobs = columns
    assert trips3 == {'part', 'full', 'many'}
    assert {G.job_trips(n, 4) for n in G.AHEAD_FLAT_COLS} == {'part'}
    assert set(G.PLAN_COLS) == {16, 17}


def test_tile_numbering_is_a_permutation():
    for nb in range(1, 2101):
        assert sorted(G.xcd_tile(b, nb) for b in range(nb)) == list(range(nb)), nb


def test_every_sample_is_covered_once():
    totals = set(G.SWEEP_TOTALS) | set(G.EDGE_TOTALS) | set(G.AHEAD_TOTALS) | set(G.HGC_TOTALS)
    totals |= {t for _, t in G.JOB_CASES}
    tails = set()
    for total in sorted(totals):
        seen = np.zeros(total, np.int64)
        for base, n in G.tiles_of(total):
            assert 0 < n <= G.gc_tile(total) and 0 <= base and base + n <= total, (total, base, n)
            seen[base:base + n] += 1
        assert (seen == 1).all(), total
        tails.add((G.gc_tile(total), total % G.gc_tile(total)))
    assert (64, 1) in tails and (4, 3) in tails and (64, 0) in tails     # a tile of 64 with a one-sample tail
    assert {len(G.tiles_of(t)) & 7 for t in totals} >= {0, 1, 3}          # grids with and without a remainder


def test_layout_guards_and_expectation():
    """The image builder: every destination has 64 sentinel bytes on both
    sides, no region overlaps, and expected_image is plain fancy indexing."""
    cols = [G.col(12, 8, 1, 32, 1), G.col(3, 1, 0, 0, 0), G.col(16, 16, 4, 32, 0)]
    R, total = 7, 5
    image, at = G.layout(cols, R, total, seed=1)
    sels = {0: np.array([6, 0, 0, 3, 6]), 1: np.array([6, 1, 1, 4, 6])}
    exp = G.expected_image(image, cols, at, sels, R, total)
    spans = []
    for c, (src_at, dst_at, pitch) in zip(cols, at):
        assert src_at % 256 == c['src_off'] and (dst_at - G.GUARD) % 256 == c['dst_off']
        n = total * c['row_bytes']
        assert (image[dst_at - G.GUARD:dst_at + n + G.GUARD] == G.SENTINEL).all()
        spans += [(src_at, src_at + (R - 1) * pitch + c['row_bytes']), (dst_at - G.GUARD, dst_at + n + G.GUARD)]
        for j, r in enumerate(sels[c['select']]):
            assert np.array_equal(exp[dst_at + j * c['row_bytes']:dst_at + (j + 1) * c['row_bytes']],
                                  image[src_at + r * pitch:src_at + r * pitch + c['row_bytes']])
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == len(image)
    changed = np.nonzero(exp != image)[0]
    assert all(any(d <= i < d + total * c['row_bytes'] for c, (_, d, _) in zip(cols, at)) for i in changed)
    idx = G.explicit_idxs(257, 192)
    assert (idx['repeats_and_last'] == 191).any() and len(set(idx['one_row'])) == 1
    assert len(set(idx['repeats_and_last'])) < 257 and G.explicit_idxs(1, 192)['repeats_and_last'][0] == 191
