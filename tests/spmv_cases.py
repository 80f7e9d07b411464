"""Seeded problems whose matrices reach the edges of the sparse-product kernels (csrc/kernels.hip k_spmv<G>, csrc/panel.hip)
at SMALL panel widths: ragged row lengths, empty rows, empty (row, panel) cells, wholly empty panels, slices of 1 / 63 /
64 / 65 rows, tiles cut by the row cap and by the non-zero budget, rows longer than the tile budget, rectangular A.

Every builder returns a Case: triu P with diagonal >= 1 + sum |off-diagonal| of its row (the setup is happy), q, A, l <= u
and the test vectors x (length n) and y (length m).  Two variants: "int" -- entries of P, A, x, y are small integers, every
partial sum far below 2^53, so any order of summation is exact -- and "real" -- row i of A is multiplied by 10^U(-6, 6)
(P: its off-diagonals by s_i s_j, s = 10^U(-3, 3)) and the vectors are standard normal.  Plain host Python; the layout
arithmetic of panel.hip that the tests need (panels, groups) is restated here from its definition."""
import functools

import numpy as np
import scipy.sparse as sp

import spmv_reference as ref

VARIANTS = ("int", "real")
LDS_SHIFTS = (6, 8)          # OSQP_AMD_PANEL_SHIFT of the LDS-panel runs: panels of 64 and 256 columns
GROUPS = (1, 2, 3, 4)        # OSQP_AMD_PANEL_GROUP
WIDE_PANEL_SHIFT = 6         # OSQP_AMD_PANEL_SHIFT of the wide runs (the threshold above which a matrix gets panels)
WIDE_SHIFTS = (7, 9)         # OSQP_AMD_WIDE_SHIFT
CSR_LANES = (1, 2, 4, 8, 16, 32, 64)
TILE_ROWS_MAX = 3968         # panel.hip kTileRowsMax
EMPTY_BLOCK = (256, 512)     # columns of `ragged` without any entry: a whole panel at width 256, four at width 64


class Case:
    def __init__(self, name, variant, P, q, A, l, u, x, y, env=None, notes=None):
        self.name, self.variant = name, variant
        self.P, self.q, self.A, self.l, self.u, self.x, self.y = P, q, A, l, u, x, y
        self.env = dict(env or {})      # settings the case needs on top of the run's (e.g. a small tile budget)
        self.notes = dict(notes or {})  # what the builder planted (row ids ...), for the structure checks
        self.n, self.m = A.shape[1], A.shape[0]

    @property
    def Pfull(self):
        return _sym_keep_zeros(self.P)

    def matrices(self, P=None, A=None):
        """op of osqp_amd_apply -> (matrix, input vector)."""
        A = self.A if A is None else A
        Pf = self.Pfull if P is None else _sym_keep_zeros(P)
        return {0: (sp.csr_matrix(A), self.x), 1: (sp.csr_matrix(A.T), self.y), 2: (Pf, self.x)}

    def products(self, P=None, A=None):
        return {op: ref.reference(M, v) for op, (M, v) in self.matrices(P, A).items()}

    def problem(self):
        return dict(P=self.P, q=self.q, A=self.A, l=self.l, u=self.u)


def _sym_keep_zeros(Pu):
    """Full symmetric matrix of an upper triangle, stored zeros kept as stored entries (the library mirrors every stored
    entry of triu P)."""
    Pu = sp.coo_matrix(Pu)
    off = Pu.row != Pu.col
    r = np.concatenate((Pu.row, Pu.col[off])); c = np.concatenate((Pu.col, Pu.row[off])); v = np.concatenate((Pu.data, Pu.data[off]))
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    indptr = np.zeros(Pu.shape[0] + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return sp.csr_matrix((v, c.astype(np.int64), np.cumsum(indptr)), shape=Pu.shape)


# ---------------------------------------------------------------------------------------------------------------------
# assembly
# ---------------------------------------------------------------------------------------------------------------------
def _values(rng, k):
    return rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=k)


def _assemble_A(rows, n, rng, variant, zeros=0):
    """rows: one sorted array of distinct column ids per row.  `zeros` stored entries get the value 0."""
    m = len(rows)
    indptr = np.zeros(m + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if indptr[-1] else np.zeros(0, dtype=np.int64)
    data = _values(rng, int(indptr[-1]))
    if zeros:
        data[rng.choice(len(data), size=zeros, replace=False)] = 0.0
    if variant == "real":
        data = data * np.repeat(10.0 ** rng.uniform(-6, 6, size=m), np.diff(indptr))
    A = sp.csr_matrix((data, indices, indptr), shape=(m, n)).tocsc()
    assert A.has_canonical_format and A.nnz == len(data)
    return A


def _make_P(n, rng, variant, long_rows=()):
    """triu P: 0-3 off-diagonals per row (plus `long_rows`: (row, columns)), diagonal = 1 + sum |off-diagonal| of the FULL row."""
    r_, c_ = [], []
    for i in range(n - 1):
        k = int(rng.integers(0, 4))
        if k:
            cols = np.unique(rng.integers(i + 1, n, size=k))
            r_.append(np.full(len(cols), i)); c_.append(cols)
    for i, cols in long_rows:
        cols = np.asarray([c for c in cols if c > i])
        r_.append(np.full(len(cols), i)); c_.append(cols)
    r = np.concatenate(r_); c = np.concatenate(c_)
    rc = np.unique(np.stack((r, c), axis=1), axis=0)
    r, c = rc[:, 0], rc[:, 1]
    v = _values(rng, len(r))
    if variant == "real":
        s = 10.0 ** rng.uniform(-3, 3, size=n)
        v = v * s[r] * s[c]
    rowsum = np.zeros(n)
    np.add.at(rowsum, r, np.abs(v)); np.add.at(rowsum, c, np.abs(v))
    diag = np.ceil(1.0 + rowsum) if variant == "int" else 1.0 + rowsum
    P = sp.coo_matrix((np.concatenate((v, diag)), (np.concatenate((r, np.arange(n))), np.concatenate((c, np.arange(n))))), shape=(n, n)).tocsc()
    P.sort_indices()
    return P


def _vectors(n, m, rng, variant):
    if variant == "int":
        return rng.integers(-4, 5, size=n).astype(np.float64), rng.integers(-4, 5, size=m).astype(np.float64)
    return rng.standard_normal(n), rng.standard_normal(m)


def _finish(name, variant, rng, n, rows, zeros=0, env=None, notes=None, P_long=()):
    A = _assemble_A(rows, n, rng, variant, zeros)
    m = A.shape[0]
    P = _make_P(n, rng, variant, P_long)
    x, y = _vectors(n, m, rng, variant)
    q = rng.integers(-3, 4, size=n).astype(np.float64)
    l = -1.0 - rng.integers(0, 3, size=m).astype(np.float64)
    u = 1.0 + rng.integers(0, 3, size=m).astype(np.float64)
    return Case(name, variant, P, q, A, l, u, x, y, env, notes)


def _pick(rng, lo, hi, k):
    """k distinct sorted columns in [lo, hi)."""
    return np.sort(rng.choice(np.arange(lo, hi), size=min(k, hi - lo), replace=False))


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged(variant="int", n=1000, m=1500, seed=11):
    """Row lengths 0 (10 % of the rows), 1, 2 and a heavy tail up to one row with an entry in every column the matrix uses
    (the columns of EMPTY_BLOCK hold no entry at all: a wholly empty panel); rows dense in exactly one panel, rows that
    live only in the first panel, rows that live only in the last (partial) panel, twelve stored zeros."""
    rng = np.random.default_rng(seed)
    e0, e1 = EMPTY_BLOCK
    allowed = np.concatenate((np.arange(0, e0), np.arange(e1, n)))
    last64 = ((n - 1) // 64) * 64   # first column of the last panel at width 64 (inside the last panel at width 256 too)
    rows = [None] * m
    ids = rng.permutation(m)
    take = iter(ids)
    notes = {"empty": [], "first_only": [], "last_only": [], "dense_in_one": {}, "dense": None}
    for _ in range(m // 10):
        i = next(take); rows[i] = np.zeros(0, dtype=np.int64); notes["empty"].append(int(i))
    notes["dense"] = int(next(take)); rows[notes["dense"]] = allowed.copy()
    # dense in exactly one panel: [576, 640) is panel 9 at width 64, [512, 768) panel 2 at width 256, [768, n) the last at 256
    for lo, hi in ((576, 640), (512, 768), (768, min(n, 1024))):
        i = int(next(take)); rows[i] = np.arange(lo, hi); notes["dense_in_one"][i] = (lo, hi)
    for _ in range(30):
        i = int(next(take)); rows[i] = _pick(rng, 0, 64, int(rng.integers(1, 21))); notes["first_only"].append(i)
    for _ in range(30):
        i = int(next(take)); rows[i] = _pick(rng, last64, n, int(rng.integers(1, 21))); notes["last_only"].append(i)
    rest = list(take)
    for j, i in enumerate(rest):
        if j % 3 == 0:
            k = 1
        elif j % 3 == 1:
            k = 2
        else:
            k = int(min(400, 3 + 4 * rng.pareto(1.1)))
        rows[i] = np.sort(rng.choice(allowed, size=k, replace=False))
    return _finish("ragged", variant, rng, n, rows, zeros=12, notes=notes, P_long=[(3, allowed[::2]), (n // 2, allowed[1::3])])


@functools.lru_cache(maxsize=None)
def many_short_rows(variant="int", n=8200, m=9000, seed=12):
    """Rows of 0, 1 or 2 entries.  Every (group, row) cell costs at least 1 and the tile budget is never below 3968, so more
    than 2 * 3968 rows are at least two tiles per group, cut by the row cap and not by the non-zero budget."""
    rng = np.random.default_rng(seed)
    rows = [_pick(rng, 0, n, int(rng.integers(0, 3))) for _ in range(m)]
    return _finish("many_short_rows", variant, rng, n, rows)


SLICE_EDGE_COUNTS = (1, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def slice_edges(variant="int", shift=6, seed=13):
    """Four panels of 2^shift columns holding exactly 1, 63, 64 and 65 non-empty rows (one slice with a single lane, one lane
    short of full, exactly full, one lane into the second slice), 1-5 entries per non-empty cell."""
    rng = np.random.default_rng(seed + shift)
    W = 1 << shift
    n, m = 4 * W, 130
    cols = [[] for _ in range(m)]
    for p, cnt in enumerate(SLICE_EDGE_COUNTS):
        for i in rng.choice(m, size=cnt, replace=False):
            cols[i].append(_pick(rng, p * W, (p + 1) * W, int(rng.integers(1, 6))))
    rows = [np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols]
    return _finish("slice_edges", variant, rng, n, rows, notes={"shift": shift})


LONG_ROWS_TILE_NNZ = 48
OVER_BUDGET_N, OVER_BUDGET_GROUP = 4400, 16  # 16 panels of 256 columns per group: 4096 columns, more than the 3968 of any budget
LONG_RUNS = ((192, 200), (0, 330), (448, 352), (37, 257), (130, 200))  # (first column, length) of the consecutive runs


@functools.lru_cache(maxsize=None)
def long_rows(variant="int", n=800, m=576, seed=14):
    """A few rows of 200-352 CONSECUTIVE columns among short ones, under OSQP_AMD_PANEL_TILE_NNZ = 48: such a row has more
    entries inside one group than the tile budget asked for, and where a run starts at a multiple of 64 (the first three)
    a panel change falls exactly on a 64-entry chunk boundary of the value refresh (k_sell_scatter); the other two change
    panel in the middle of a chunk.  One row holds every column."""
    rng = np.random.default_rng(seed)
    rows = [_pick(rng, 0, n, int(rng.integers(0, 13))) for _ in range(m)]
    ids = rng.choice(m, size=len(LONG_RUNS) + 1, replace=False)
    runs = {}
    for i, (c0, k) in zip(ids, LONG_RUNS):
        rows[i] = np.arange(c0, c0 + k); runs[int(i)] = (c0, k)
    rows[ids[-1]] = np.arange(n)
    return _finish("long_rows", variant, rng, n, rows, env={"OSQP_AMD_PANEL_TILE_NNZ": str(LONG_ROWS_TILE_NNZ)},
                   notes={"runs": runs, "dense": int(ids[-1])})


@functools.lru_cache(maxsize=None)
def flat(variant="int", n=1000, m=40, seed=15):
    """m = 40 <= W < n: A (40 x n) runs on panels, A' (n x 40) has too few columns for one and stays on the CSR kernel."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(m):
        k = 0 if i % 10 == 3 else (n if i == 7 else int(min(n, 1 + i * i)))
        rows.append(_pick(rng, 0, n, k))
    return _finish("flat", variant, rng, n, rows)


def unroll_lengths():
    out = set()
    for G in CSR_LANES:
        out.update((0, 1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G + 3))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def unroll_edges(variant="int", n=600, seed=16):
    """Row lengths 0, 1, G-1, G, G+1, 4G-1, 4G, 4G+1, 8G+3 for every lane width G of k_spmv<G>, three rows of each, mixed:
    the 4G unroll test, the tail loop and rows shorter than G, whatever G the run forces."""
    rng = np.random.default_rng(seed)
    lens = np.repeat(unroll_lengths(), 3)
    rng.shuffle(lens)
    rows = [_pick(rng, 0, n, int(k)) for k in lens]
    return _finish("unroll_edges", variant, rng, n, rows, notes={"lengths": [int(k) for k in lens]})


BUILDERS = {"ragged": ragged, "many_short_rows": many_short_rows, "slice_edges": slice_edges, "long_rows": long_rows,
            "flat": flat, "unroll_edges": unroll_edges}


def build(name, variant, shift=None, **kw):
    if name == "slice_edges":
        return slice_edges(variant, shift if shift is not None else 6)
    return BUILDERS[name](variant, **kw)


# the runs of the GPU test: (builder, builder arguments, panel shift)
LDS_RUNS = [(name, (), shift) for shift in LDS_SHIFTS for name in BUILDERS] + [("ragged", (("n", 5000),), 6)]
WIDE_RUNS = [(name, (), ws) for ws in WIDE_SHIFTS for name in ("ragged", "many_short_rows")]
CSR_RUNS = [(name, (), G) for G in CSR_LANES for name in ("unroll_edges", "ragged")]


# ---------------------------------------------------------------------------------------------------------------------
# the layout arithmetic of panel.hip, restated
# ---------------------------------------------------------------------------------------------------------------------
def expected_layout(cols, mode, shift, group, wide_shift=None):
    """kernel (0 CSR / 2 LDS panels / 3 wide), panel shift, B, Gp, NG for a matrix of `cols` columns under OSQP_AMD_PANEL =
    mode, OSQP_AMD_PANEL_SHIFT = shift, OSQP_AMD_PANEL_GROUP = group (OSQP_AMD_WIDE_SHIFT = wide_shift in mode 3): a matrix
    gets panels when it has more columns than one panel of 2^shift."""
    if mode == 0 or cols <= (1 << shift):
        return dict(kernel=0, shift=0, B=0, Gp=0, NG=0)
    s = shift if mode == 2 else wide_shift
    B = (cols + (1 << s) - 1) >> s
    Gp = min(group, B)
    return dict(kernel=mode, shift=s, B=B, Gp=Gp, NG=(B + Gp - 1) // Gp)


def structure(M, shift):
    """Pattern facts of M at panel width 2^shift: cell[i, b] = stored entries of row i inside panel b, and what follows."""
    M = sp.csr_matrix(M)
    rows, cols = M.shape
    B = (cols + (1 << shift) - 1) >> shift
    r = np.repeat(np.arange(rows), np.diff(M.indptr))
    cell = np.zeros((rows, B), dtype=np.int64)
    np.add.at(cell, (r, M.indices >> shift), 1)
    width = np.minimum((np.arange(B) + 1) << shift, cols) - (np.arange(B) << shift)
    return dict(B=B, cell=cell, width=width, empty_rows=int(np.sum(cell.sum(axis=1) == 0)), empty_cells=int(np.sum(cell == 0)),
                empty_panels=[int(b) for b in np.nonzero(cell.sum(axis=0) == 0)[0]], rows_in_panel=(cell > 0).sum(axis=0),
                nnz=int(M.nnz))
