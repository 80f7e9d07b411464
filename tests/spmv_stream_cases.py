"""Seeded problems for the per-lane slice table of the panel product (csrc/panel.hip: slice_rows holds, per lane, the row
inside the tile as 16 bits; 0xFFFF marks an empty lane) and for the way the product streams a slice (OSQP_AMD_SELL_NT):
slices whose rows fall far short of the slice's length, slices that end on, one past and one short of a full batch of 16
positions, a slice of a single lane, the largest row id a tile can hold.  Same Case objects, variants and exact reference as
spmv_cases.py; the layout panel.hip gives each case (slices of 64 rows sorted longest first inside a tile and panel) is
restated here by `slices_of`, so that a test can assert the case really has the slices it is there for.

Layout facts the builders rely on (panel.hip): a matrix this small is one tile per group unless a budget is set; inside a
(tile, panel) unit the non-empty rows are sorted by their length inside the panel, longest first, ties by row id, and cut
into slices of 64; a slice is as long as its first row."""
import functools

import numpy as np
import scipy.sparse as sp

import spmv_cases as sc

SHIFT = 8                      # 256-column panels
W = 1 << SHIFT
GROUPS = (1, 2)
LADDER = [40 - (i * 40) // 64 for i in range(64)]   # 40, 40, 39, ... , 1: every length from 40 down to 1
SECOND = [16] * 63 + [15]                           # a slice of exactly one full batch, its last lane one short
LONE = [40 - (i % 7) for i in range(64)] + [33]     # 64 rows of 34 .. 40 entries, then one of 33: a slice of a single lane
TILE_ROWS = sc.TILE_ROWS_MAX
LAST_ROW_TILE_NNZ = 17 * TILE_ROWS                  # cost floor of a (group, row) cell = 17 (34 with two panels per group): exactly 3968 rows per tile
LAST_ROW_PANEL = 3                                  # the 64-column panel that holds the long row and the tile's last row


def slices_of(M, shift, r0=0, r1=None):
    """{panel: [lengths of slice 0, lengths of slice 1, ...]} for rows [r0, r1) of M taken as ONE tile."""
    M = sp.csr_matrix(M)
    r1 = M.shape[0] if r1 is None else r1
    cell = sc.structure(M, shift)["cell"][r0:r1]
    out = {}
    for b in range(cell.shape[1]):
        ids = np.nonzero(cell[:, b])[0]
        order = ids[np.lexsort((ids, -cell[ids, b]))]
        lens = cell[order, b]
        out[b] = [lens[k:k + 64].tolist() for k in range(0, len(lens), 64)]
    return out


def padded_of(slices):
    return int(sum(64 * s[0] for per_panel in slices.values() for s in per_panel))


def _filler(rng, rows, lo, hi, count):
    """`count` more rows with 1-5 entries in columns [lo, hi): they keep A' and P on panels and touch no other panel."""
    for _ in range(count):
        rows.append(sc._pick(rng, lo, hi, int(rng.integers(1, 6))))


@functools.lru_cache(maxsize=None)
def ladder(variant="int", seed=31):
    """A is 320 x 768, three panels of 256 columns.  Rows 0..63: 40, 40, 39, ..., 1 entries inside panel 0 (slice_len 40 crosses
    the batch boundaries at 16 and 32; the rows fall 0 .. 39 entries short of it) and 17 inside panel 1 (no row short, one
    position past a full batch).  Rows 64..127: nothing in panel 0, and 16, 16, ..., 15 entries inside panel 1 -- the
    second slice of the panel-1 unit, behind the slice of 17s (the rows of a unit are sorted longest first, so a 16-long
    slice cannot follow the ladder, which ends at length 1, inside the panel-0 unit).  Rows 128..319: 1-5 entries in panel 2."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(64):
        rows.append(np.concatenate((sc._pick(rng, 0, W, LADDER[i]), sc._pick(rng, W, 2 * W, 17))))
    for i in range(64):
        rows.append(sc._pick(rng, W, 2 * W, SECOND[i]))
    _filler(rng, rows, 2 * W, 3 * W, 192)
    case = sc._finish("ladder", variant, rng, 3 * W, rows)
    s = slices_of(case.A, SHIFT)
    assert s[0] == [LADDER] and s[1] == [[17] * 64, SECOND] and all(len(x) <= 64 for x in s[2])
    return case


@functools.lru_cache(maxsize=None)
def lone_row(variant="int", seed=32):
    """65 non-empty rows in panel 0: 64 of 34 .. 40 entries and one of 33 -- the second slice has one row and 63 empty lanes,
    slice_len 33 (two full batches and one position).  Rows 65..299: 1-5 entries in panel 1."""
    rng = np.random.default_rng(seed)
    rows = [sc._pick(rng, 0, W, k) for k in LONE]
    _filler(rng, rows, W, 2 * W, 235)
    case = sc._finish("lone_row", variant, rng, 2 * W, rows)
    s = slices_of(case.A, SHIFT)
    assert len(s[0]) == 2 and s[0][1] == [33] and s[0][0][0] == 40
    return case


@functools.lru_cache(maxsize=None)
def last_local_row(variant="int", seed=33):
    """A is 7936 x 512 at 64-column panels under OSQP_AMD_PANEL_TILE_NNZ = 17 * 3968: every (group, row) cell costs the floor
    (17 entries, or 34 with two panels per group), so the tiles are rows [0, 3968) and [3968, 7936).  Rows have 1-2
    entries outside panel 3; inside panel 3 only row 5 (17 entries), ten rows of 1-2 and row 3967 (one entry) have any:
    one slice, slice_len 17, whose last lane holds local row 3967 = 0x0F7F, the largest entry the table can hold, next to
    0xFFFF in the empty lanes behind it.  x is non-zero at that entry's column, so a lane taken for empty changes row 3967."""
    rng = np.random.default_rng(seed)
    n, m, p = 512, 2 * TILE_ROWS, LAST_ROW_PANEL
    outside = np.concatenate((np.arange(0, 64 * p), np.arange(64 * (p + 1), n)))
    rows = [np.sort(rng.choice(outside, size=int(rng.integers(1, 3)), replace=False)) for _ in range(m)]
    rows[5] = sc._pick(rng, 64 * p, 64 * (p + 1), 17)
    for i in rng.choice(np.arange(100, 3900), size=10, replace=False):
        rows[i] = sc._pick(rng, 64 * p, 64 * (p + 1), int(rng.integers(1, 3)))
    col = 64 * p + 21
    rows[TILE_ROWS - 1] = np.array([col])
    case = sc._finish("last_local_row", variant, rng, n, rows, env={"OSQP_AMD_PANEL_TILE_NNZ": str(LAST_ROW_TILE_NNZ)},
                      notes={"row": TILE_ROWS - 1, "col": col})
    case.x = case.x.copy()
    case.x[col] = 3.0
    assert case.A[TILE_ROWS - 1, col] != 0.0
    s = slices_of(case.A, 6, 0, TILE_ROWS)[p]
    assert len(s) == 1 and s[0][0] == 17 and s[0][-1] == 1 and len(s[0]) == 12
    return case
