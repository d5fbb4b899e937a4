"""The samplers' shared row gather (copy_tile / copy_rows of
ogbench_amd/csrc/gc_device.h), restated from the header's comments in plain
Python / NumPy, and the case matrix that tests/test_gather_gpu.py drives and
tests/test_gather_cpu.py proves complete.  Nothing here calls the library.

The rules
    gc_tile(total)      samples per workgroup: total // 1024 clamped to [1, 64].
    xcd_tile(b, nb)     workgroup b of nb owns tile x * (nb >> 3) + min(x, nb & 7)
                        + (b >> 3) with x = b & 7 (XCD-major numbering).
    copy_unit(...)      the widest W of {16, 8, 4, 1} with row_bytes % W == 0 and
                        (src | dst | src_stride) % W == 0.
    flat4_table(cols)   every column has row_bytes % 4 == 0, row_bytes <= 512 and
                        (src | dst | src_stride) % 4 == 0.  The tiled kernels take
                        the per-wave job copy when this holds and tile <= 4
                        (total < 5120); the look-ahead kernels (tile 1) when it
                        holds.
    job copy            a (column, sample) row is one job; the copying waves
                        (4, or 3 with the first wave left out) take 8 jobs each
                        per trip, so a full trip is 32 jobs (24 with 3 waves).
    expected(src, sel, row_bytes, stride)  rows sel of a source whose rows lie
                        stride bytes apart (0: dense).

A column spec is a dict(row_bytes, src_off, dst_off, stride, select); layout()
places every column's source and destination inside one byte image whose base
the GPU test asserts to be 256-aligned, so the offsets alone decide the unit.
"""

import numpy as np

MAX_TILE = 64
FLAT_MAX_ROW = 512
FLAT_MAX_TILE = 4
JOBS_PER_WAVE = 8
SENTINEL = 0xA5
GUARD = 64

# ---------------------------------------------------------------- the rules


def gc_tile(total):
    return min(max(total // 1024, 1), MAX_TILE)


def xcd_tile(b, nb):
    per, rem, x = nb >> 3, nb & 7, b & 7
    return x * per + min(x, rem) + (b >> 3)


def tiles_of(total):
    """(base, n_here) of every workgroup of a tiled launch, in workgroup order."""
    tile = gc_tile(total)
    nb = (total + tile - 1) // tile
    out = []
    for b in range(nb):
        base = xcd_tile(b, nb) * tile
        out.append((base, min(tile, total - base)))
    return out


def copy_unit(row_bytes, src, dst, src_stride):
    align = src | dst | src_stride
    return next(w for w in (16, 8, 4, 1) if row_bytes % w == 0 and align % w == 0)


def spec_unit(c):
    return copy_unit(c['row_bytes'], c['src_off'], c['dst_off'], c['stride'])


def flat4_table(cols):
    return all(c['row_bytes'] % 4 == 0 and c['row_bytes'] <= FLAT_MAX_ROW and
               (c['src_off'] | c['dst_off'] | c['stride']) % 4 == 0 for c in cols)


def flat4_tiled(cols, total):
    """The tiled kernels (ogbx_gc_sample, ogbx_hgc_sample, ogbx_replay_sample)."""
    return gc_tile(total) <= FLAT_MAX_TILE and flat4_table(cols)


def job_trips(jobs, waves):
    """'part': one trip that is not full, 'full': exactly one full trip, 'many'."""
    full = waves * JOBS_PER_WAVE
    return 'part' if jobs < full else 'full' if jobs == full else 'many'


def units_class(units):
    """One unit per row, several handled in one pass of the 192 / 256 copying
    threads, or more units than threads (the loop's k / b carry)."""
    return 'one' if units == 1 else 'several' if units <= 192 else 'above256' if units > 256 else 'between'


def expected(src, sel, row_bytes, stride=0):
    """Rows sel of a source given as bytes from its row 0 on, stride bytes
    apart (0: dense): NumPy fancy indexing on a [rows, row_bytes] view."""
    pitch = stride or row_bytes
    sel = np.asarray(sel, np.int64)
    num_rows = (len(src) - row_bytes) // pitch + 1
    assert sel.min() >= 0 and sel.max() < num_rows
    rows = np.lib.stride_tricks.as_strided(src, (num_rows, row_bytes), (pitch, 1), writeable=False)
    return rows[sel]


# ---------------------------------------------------------------- the byte image


def col(row_bytes, src_off=0, dst_off=0, stride=0, select=0):
    return dict(row_bytes=row_bytes, src_off=src_off, dst_off=dst_off, stride=stride, select=select)


def _up(x, a=256):
    return (x + a - 1) // a * a


_POOL = np.random.default_rng(20).integers(0, 256, 1 << 23, dtype=np.uint8)


def _random_bytes(n, key):
    """n bytes of a fixed random pool, from a start that the key picks (a
    source is far smaller than the pool; drawing each one afresh costs more
    than the gather under test)."""
    assert n < len(_POOL) // 2
    at = key % (len(_POOL) - n)
    return _POOL[at:at + n]


def layout(cols, num_rows, total, seed=0):
    """One uint8 image holding every column's source (num_rows rows at its
    pitch, random bytes, the gaps of a strided source included) and destination
    (total rows, GUARD sentinel bytes and more on each side).  Returns
    (image, [(src_at, dst_at, pitch)])."""
    at, cur = [], 0
    for c in cols:
        pitch = c['stride'] or c['row_bytes']
        assert pitch >= c['row_bytes']
        src_at = _up(cur) + c['src_off']
        cur = src_at + (num_rows - 1) * pitch + c['row_bytes']
        at.append([src_at, None, pitch])
    src_end = cur
    for c, a in zip(cols, at):
        a[1] = _up(cur) + GUARD + c['dst_off']
        cur = a[1] + total * c['row_bytes'] + GUARD
    image = np.full(cur, SENTINEL, np.uint8)
    for i, (c, (src_at, _, pitch)) in enumerate(zip(cols, at)):
        n = (num_rows - 1) * pitch + c['row_bytes']
        image[src_at:src_at + n] = _random_bytes(n, seed * 7919 + i * 104729)
    assert all(a[0] + (num_rows - 1) * a[2] + c['row_bytes'] <= src_end for c, a in zip(cols, at))
    return image, [tuple(a) for a in at]


def expected_image(image, cols, at, sels, num_rows, total):
    """The image after a correct gather: every destination holds
    source[sels[select]], everything else is untouched."""
    exp = image.copy()
    for c, (src_at, dst_at, pitch) in zip(cols, at):
        sel = np.asarray(sels[c['select']], np.int64)
        assert sel.shape == (total,) and sel.min() >= 0 and sel.max() < num_rows
        src = image[src_at:src_at + (num_rows - 1) * pitch + c['row_bytes']]
        rows = expected(src, sel, c['row_bytes'], c['stride'])
        exp[dst_at:dst_at + total * c['row_bytes']] = rows.reshape(-1)
    return exp


# ---------------------------------------------------------------- the matrix
# Width x alignment x stride (ogbx_replay_sample with explicit idxs, 16-entry
# table, selectors 0-1; ogbx_gc_sample with injected idxs, 32-entry table,
# selectors 0-3).

ROW_BYTES = (1, 3, 4, 8, 12, 16, 20, 24, 48, 116, 232, 256, 260, 276, 508, 512, 516, 520, 528, 1608, 12288, 259)
OFFSETS = ((0, 0), (8, 8), (4, 4), (1, 1), (0, 4), (8, 0), (16, 1))   # the ingest sweep's set
STRIDE_PADS = (None, 0, 4, 8, 16)                                   # None: src_stride 0 (dense)
SWEEP_TOTALS = (1, 3, 64, 257)
ENTRY_TABLE = {'replay': (16, 2), 'gc': (32, 4)}                    # entry point -> (table entries, selectors)


def sweep_combos(row_bytes):
    """Every (src_off, dst_off, stride) of a row size; 12-byte rows also as the
    packed record: a 12-byte column at offset 8 of a 32-byte record."""
    out = [(so, do, 0 if pad is None else row_bytes + pad) for so, do in OFFSETS for pad in STRIDE_PADS]
    if row_bytes == 12:
        out += [(8, do, 32) for do in (0, 4, 8, 1)]
    return out


def sweep_tables(row_bytes, entry):
    """The column tables of one row size for one entry point: first the
    4-byte-granular combinations alone (a flat table where the row allows it),
    then every combination in table-sized chunks, each chunk opened by an odd
    destination so that it is not flat whatever else it holds."""
    size, nsel = ENTRY_TABLE[entry]
    combos = sweep_combos(row_bytes)
    mk = lambda group: [col(row_bytes, so, do, st, i % nsel) for i, (so, do, st) in enumerate(group)]
    tables = []
    granular = [c for c in combos
                if row_bytes % 4 == 0 and row_bytes <= FLAT_MAX_ROW and (c[0] | c[1] | c[2]) % 4 == 0]
    for i in range(0, len(granular), size):
        tables.append(mk(granular[i:i + size]))
    odd = (16, 1, 0)
    for i in range(0, len(combos), size - 1):
        tables.append(mk([odd] + combos[i:i + size - 1]))
    return tables


# Tile and grid edges (ogbx_gc_sample, injected and Philox instance).
EDGE_TOTALS = (1, 7, 8, 9, 1023, 1024, 1025, 2053, 4099, 5119, 5120, 65536, 65537)
EDGE_LARGE = 65536   # from here on: at most three narrow columns


def edge_tables(total):
    """A flat-eligible table, one with a 1-byte column and, below the two
    largest totals, one of wide rows: copy_rows carries from one row of a tile
    into the next only where a tile has several samples, and with more units
    per row than threads only there, which the width sweep (tile 1) cannot
    reach."""
    if total >= EDGE_LARGE:
        return {'flat': [col(4, select=0), col(12, 4, 4, 16, 2), col(20, 0, 4, 0, 1)],
                'byte': [col(4, select=0), col(12, 4, 4, 16, 2), col(1, 0, 0, 0, 3)]}
    flat = [col(4, select=0), col(12, 8, 4, 32, 3), col(276, 4, 0, 0, 1), col(512, 0, 0, 0, 2)]
    wide = [col(4112, 0, 0, 0, 0), col(2056, 8, 8, 2064, 1), col(1608, 4, 4, 0, 2), col(259, 0, 1, 0, 3),
            col(800, 4, 4, 0, 1), col(12, 4, 0, 0, 2), col(3, 1, 0, 4, 0)]     # 257, 257, 402, 259, 200, 3, 3 units
    return {'flat': flat, 'byte': flat + [col(1, 0, 0, 0, 1)], 'wide': wide}


# Job loop (ogbx_gc_sample; flat tables): (columns, total).  Totals 1 and 3 run
# tile 1, total 4099 tile 4 with a last tile of 3 samples.
JOB_ROWS = (4, 12, 8, 16, 20, 48, 116, 260, 512, 24, 232)
JOB_CASES = ((24, 1), (25, 1), (32, 1), (8, 4099), (11, 4099), (9, 4099), (32, 4099),
             (1, 3), (9, 3), (16, 3), (17, 3), (32, 3), (1, 4099), (16, 4099), (17, 4099))


def flat_table(num_cols, nsel, rows=JOB_ROWS):
    offs = ((0, 0), (4, 8), (8, 8), (16, 0), (4, 4))
    pads = (None, 0, 4, 8, 16)
    out = []
    for i in range(num_cols):
        rb = rows[i % len(rows)]
        so, do = offs[i % len(offs)]
        pad = pads[(i // 2) % len(pads)]
        out.append(col(rb, so, do, 0 if pad is None else rb + pad, i % nsel))
    assert flat4_table(out)
    return out


def job_counts(num_cols, total):
    """num_cols x n_here of every workgroup of the launch."""
    return sorted({num_cols * n for _, n in tiles_of(total)})


# Look-ahead kernels (tile 1; miss without ahead_out: 4 copying waves, miss
# with ahead_out and hit: 3).
AHEAD_TOTALS = (1, 5, 1024)
AHEAD_FORMS = {'miss': 0, 'miss_out': 1, 'hit': 1}   # form -> wave0
AHEAD_FLAT_COLS = (9, 24, 25)                       # below, exactly and above one full trip of 3 waves


def ahead_nonflat_table(nsel):
    """Every unit with one unit per row, several, and more than 256."""
    specs = [(16, 0, 0, 0), (48, 0, 0, 64), (12288, 0, 0, 0),       # 16: 1, 3, 768 units
             (8, 8, 8, 0), (24, 8, 0, 32), (2056, 8, 8, 0),         # 8: 1, 3, 257
             (4, 4, 4, 0), (12, 8, 4, 32), (1028, 4, 0, 1032),      # 4: 1, 3, 257
             (1, 1, 1, 0), (3, 0, 1, 4), (259, 0, 0, 0)]            # 1: 1, 3, 259
    return [col(rb, so, do, st, i % nsel) for i, (rb, so, do, st) in enumerate(specs)]


PLAN_COLS = (16, 17)   # the 16-entry table and the 32-entry one
HGC_TOTALS = (3, 4099, 5120)


def hgc_table(flat):
    """Columns on all ten selectors; the non-flat one adds a byte column."""
    t = flat_table(10, 10, rows=(4, 12, 276, 8, 16, 48, 116, 20, 512, 24))
    return t if flat else t + [col(3, 1, 1, 0, 9), col(1608, 4, 4, 0, 5)]


def reach(cols, flat, wave0):
    """What a launch of this table reaches: (unit, units class, flat, wave0) per column."""
    return {(spec_unit(c), units_class(c['row_bytes'] // spec_unit(c)), flat, wave0) for c in cols}


def feasible_reach():
    """Every combination that exists: the flat path needs 4-byte-granular rows
    of at most 512 B, so it has no byte unit and no row above 256 units."""
    out = set()
    for wave0 in (0, 1):
        for w in (16, 8, 4, 1):
            for cls in ('one', 'several', 'above256'):
                out.add((w, cls, False, wave0))
            if w != 1:
                for cls in ('one', 'several'):
                    out.add((w, cls, True, wave0))
    return out


def explicit_idxs(total, num_rows):
    """Explicit sample rows: a pattern with repeats that visits the last row
    (the clamp of next), and one row for the whole batch."""
    a = np.arange(total, dtype=np.int64)
    mixed = (a * 7 + 3) % max(1, num_rows // 2)
    mixed[::5] = num_rows - 1
    return {'repeats_and_last': mixed, 'one_row': np.full(total, num_rows // 3, np.int64)}
