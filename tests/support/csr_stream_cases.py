"""Catalogue of the CSR-stream SpMV / SpMM tests - TEST INFRASTRUCTURE ONLY, shares no code with the package
(tests/test_csr_stream_host.py, tests/test_gpu_csr_stream.py).

Two things live here.

(i) A restatement of the host-side plan of ``kh_csr_upload``: ``rowblocks`` is the greedy rule of the row blocks (consecutive
rows while their entries fit the tile, at most 1024 rows, a row longer than the tile on its own) and ``window_plan`` the
decision about the LDS window of x (a block fits when it has at most ``tile`` entries within at most 4096 columns; the window
is on when nine blocks in ten fit, as wide as the widest block that fits).

(ii) Named structures, built for a tile ``T`` from a seeded generator.  Each states the property it exists for as a predicate
over ``window_plan`` (``Case.holds``): a structure that stops selecting what it claims fails on the CPU, before any kernel
runs.  Entry magnitudes lie in [1, 2) with random signs (a dropped or doubled product moves a row sum by at least 1), rows are
sorted, there are no stored zeros.  The one exception is ``banded_on_stream``, the five-point Laplacian every benchmark uses.
"""
import functools

import numpy as np
import scipy.sparse as sp

TILES = (1024, 2048, 4096)
ZTILES = (1024, 2048)          # complex products are (re, im) pairs: the complex kernel's tile stops at 2048
WIN_CAP = 4096                 # widest LDS window of x
MAX_ROWS = 1024                # rows per block: four per lane of a 256-lane workgroup
LANES = 256
U = 2.0 ** -53


def gamma(m):
    """``m u / (1 - m u)``: the relative error bound of a sum of ``m`` terms in ANY order."""
    return m * U / (1.0 - m * U)


# ---- the plan ---------------------------------------------------------------------------------------------------------
def rowblocks(indptr, tile):
    """Block borders ``[0, ..., n_rows]`` of the greedy rule."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = indptr.size - 1
    out = [0]
    r = 0
    while r < n:
        end = r
        while end < n and end - r < MAX_ROWS and indptr[end + 1] - indptr[r] <= tile:
            end += 1
        if end == r:           # a row longer than the tile
            end = r + 1
        out.append(end)
        r = end
    return np.array(out, dtype=np.int64)


def window_plan(A, tile):
    """``dict(blocks=[(nnz, cmin, span, fits), ...], borders, fit, nblk, widest, window_on)`` of a CSR matrix."""
    A = sp.csr_matrix(A)
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    borders = rowblocks(indptr, tile)
    blocks = []
    fit, widest = 0, 0
    for b in range(borders.size - 1):
        z0, z1 = indptr[borders[b]], indptr[borders[b + 1]]
        nnz = int(z1 - z0)
        cmin = int(indices[z0:z1].min()) if nnz else 0
        span = int(indices[z0:z1].max()) - cmin + 1 if nnz else 0
        fits = nnz <= tile and span <= WIN_CAP
        if fits:
            fit += 1
            widest = max(widest, span)
        blocks.append((nnz, cmin, span, fits))
    nblk = len(blocks)
    on = nblk > 0 and A.nnz > 0 and fit * 10 >= nblk * 9 and widest > 0
    return dict(blocks=blocks, borders=borders, fit=fit, nblk=nblk, widest=widest, window_on=on)


# ---- building blocks --------------------------------------------------------------------------------------------------
def signed(rng, shape):
    """Magnitudes in [1, 2), random signs."""
    return rng.uniform(1.0, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)


def csigned(rng, shape):
    """Complex numbers whose real and imaginary parts both have magnitudes in [1, 2) and random signs."""
    return signed(rng, shape) + 1j * signed(rng, shape)


def _strata(rng, nrows, k, width):
    """``k`` distinct ascending offsets in [0, width) per row: one at a random place of each of ``k`` equal strata."""
    step = width // k
    return np.arange(k, dtype=np.int64)[None, :] * step + rng.integers(0, step, size=(nrows, k))


def _band_rows(rng, n_rows, n_cols, k=8, half=900, shift=0):
    """Per row ``k`` sorted distinct columns at random places of the band [i + shift - half, i + shift + half), moved inside
    [0, n_cols) where it sticks out."""
    lo = np.clip(np.arange(n_rows, dtype=np.int64) + shift - half, 0, n_cols - 2 * half)
    return lo[:, None] + _strata(rng, n_rows, k, 2 * half)


def _assemble(rows, n_cols, rng, cplx=False):
    """CSR from a list of sorted column arrays, one per row, with fresh values."""
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = (np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if lens.sum() else np.zeros(0)).astype(np.int32)
    data = csigned(rng, indices.size) if cplx else signed(rng, indices.size)
    A = sp.csr_matrix((data, indices, indptr), shape=(len(rows), n_cols))
    assert A.has_sorted_indices and np.all(np.diff(A.indptr) == lens)
    for r in rows:
        assert len(r) < 2 or np.all(np.diff(np.asarray(r)) > 0), "columns of a row must ascend strictly"
    assert np.all(A.data != 0)
    return A


class Case(object):
    """One structure at one tile: the matrix, the rows that are longer than the tile (the only rows a test may treat
    differently), the switches the run needs and the property, as text and as a predicate over ``window_plan``."""

    def __init__(self, name, tile, A, claim, predicate, switches=None):
        self.name, self.tile, self.A, self.claim, self._predicate = name, tile, A, claim, predicate
        self.switches = dict(switches or {})
        self.long_rows = np.nonzero(np.diff(A.indptr) > tile)[0]
        self.plan = window_plan(A, tile)

    def holds(self, plan=None):
        return bool(self._predicate(self.plan if plan is None else plan, self))

    def __repr__(self):
        return "%s@%d" % (self.name, self.tile)


def _all_fit_rows(T, seed=1):
    rng = np.random.default_rng(seed + T)
    n = 40 * T // 8
    return [r for r in _band_rows(rng, n, n)], n, rng


def _widen(rows, T, nblocks, n):
    """The last entry of the first row of blocks 0 .. nblocks-1 moves to the far end of the matrix."""
    for b in range(nblocks):
        r = b * (T // 8)
        rows[r] = rows[r].copy()
        rows[r][-1] = n - 1 - b
    return rows


def _block_lens(c):
    return np.diff(c.plan["borders"])


def _row_lens(c):
    return np.diff(c.A.indptr)


def _is_full_tile_blocks(p, c):
    return p["nblk"] == 40 and all(b[0] == c.tile for b in p["blocks"])


# ---- the structures ---------------------------------------------------------------------------------------------------
def all_fit(T, cplx=False):
    rows, n, rng = _all_fit_rows(T)
    return Case("all_fit", T, _assemble(rows, n, rng, cplx),
                "40 blocks of exactly T entries, every one within an LDS window of 1,900 to 2,300 columns",
                lambda p, c: _is_full_tile_blocks(p, c) and p["fit"] == 40 and p["window_on"] and 1900 <= p["widest"] <= 2320 and
                c.long_rows.size == 0)


def nine_of_ten(T):
    rows, n, rng = _all_fit_rows(T)
    return Case("nine_of_ten", T, _assemble(_widen(rows, T, 4, n), n, rng),
                "36 of 40 blocks fit: the window is on and blocks 0 to 3 gather from global memory inside the window launch",
                lambda p, c: _is_full_tile_blocks(p, c) and p["fit"] == 36 and p["window_on"] and
                [b[3] for b in p["blocks"]] == [False] * 4 + [True] * 36 and all(b[2] > p["widest"] for b in p["blocks"][:4]))


def below_nine_of_ten(T):
    rows, n, rng = _all_fit_rows(T)
    return Case("below_nine_of_ten", T, _assemble(_widen(rows, T, 5, n), n, rng),
                "35 of 40 blocks fit: one short of nine in ten, the window is off",
                lambda p, c: _is_full_tile_blocks(p, c) and p["fit"] == 35 and not p["window_on"])


def _span_edge(T, span):
    rows, n, rng = _all_fit_rows(T)
    b0 = 39 * (T // 8)
    cmax = max(int(r[-1]) for r in rows[b0:])
    last = rows[n - 1].copy()
    last[0] = cmax - (span - 1)            # below every column of the block: its new leftmost one
    assert last[0] >= 0 and last[0] < last[1] and last[0] < min(int(r[0]) for r in rows[b0:n - 1])
    rows[n - 1] = last
    return rows, n, rng


def span_4096(T):
    rows, n, rng = _span_edge(T, 4096)
    return Case("span_4096", T, _assemble(rows, n, rng),
                "the last block spans exactly 4096 columns: it fits and sets the window's width (with T = 4096: 64 KB of LDS)",
                lambda p, c: _is_full_tile_blocks(p, c) and p["fit"] == 40 and p["window_on"] and p["widest"] == 4096 and
                p["blocks"][39][2] == 4096 and max(b[2] for b in p["blocks"][:39]) < 2400)


def span_4097(T):
    rows, n, rng = _span_edge(T, 4097)
    return Case("span_4097", T, _assemble(rows, n, rng),
                "the last block spans 4097 columns: it does not fit and the window is as wide as the next widest block",
                lambda p, c: _is_full_tile_blocks(p, c) and p["fit"] == 39 and p["window_on"] and p["blocks"][39][2] == 4097 and
                not p["blocks"][39][3] and p["widest"] == max(b[2] for b in p["blocks"][:39]) and p["widest"] < 2400)


def _full_row(T, window, cplx, nblocks=40):
    rng = np.random.default_rng(7 + T + (0 if window else 100))
    n = max(nblocks * T // 8, 5120)
    if window:
        rows = [r for r in _band_rows(rng, n, n)]
    else:                                  # eight entries per row anywhere in the matrix: no block within 4096 columns
        rows = [r for r in _strata(rng, n, 8, n)]
    # a row of exactly T entries within 4096 columns (T = 4096: every one of them), a block of its own that fits the window
    r_full, r_long = 11 * (T // 8) + 3, 23 * (T // 8) + 5
    if nblocks < 24:
        r_full, r_long = 2 * (T // 8) + 3, 5 * (T // 8) + 5
    rows[r_full] = 500 + np.sort(rng.choice(WIN_CAP, size=T, replace=False)).astype(np.int64)
    rows[r_long] = np.sort(rng.choice(n, size=T + 1, replace=False)).astype(np.int64)
    name = "full_row_win" if window else "full_row_nowin"

    def pred(p, c):
        lens, blen = _row_lens(c), _block_lens(c)
        b_full = int(np.searchsorted(p["borders"], r_full, side="right")) - 1
        b_long = int(np.searchsorted(p["borders"], r_long, side="right")) - 1
        ok = lens[r_full] == c.tile and lens[r_long] == c.tile + 1 and list(c.long_rows) == [r_long]
        ok = ok and blen[b_full] == 1 and blen[b_long] == 1 and p["blocks"][b_full][0] == c.tile and not p["blocks"][b_long][3]
        if window:
            return ok and p["window_on"] and p["blocks"][b_full][3] and 0 < p["fit"] < p["nblk"]
        return ok and not p["window_on"]

    return Case(name, T, _assemble(rows, n, rng, cplx),
                "a row of exactly T entries (a block of its own, every LDS slot used, bit-ordered) and a row of T + 1 entries "
                "(the tree-reduced path); window %s" % ("on" if window else "off"), pred)


def full_row_win(T, cplx=False):
    return _full_row(T, True, cplx)


def full_row_nowin(T, cplx=False):
    return _full_row(T, False, cplx, nblocks=8)


def many_short_rows(T, cplx=False):
    rng = np.random.default_rng(13 + T)
    n_one, n_empty, n_few = 1100, 2200, 3000       # (2200: a whole block of empty rows whatever the run starts in)
    n = n_one + n_empty + n_few + n_one
    rows = []

    def near(i, k):                        # k distinct columns at scattered places within 1,500 columns of the row
        lo = int(np.clip(i - 1500, 0, n - 3000))
        return lo + np.sort(rng.choice(3000, size=k, replace=False)).astype(np.int64)

    for i in range(n_one):
        rows.append(near(i, 1))
    for i in range(n_empty):
        rows.append(np.zeros(0, dtype=np.int64))
    for i in range(n_few):
        rows.append(near(n_one + n_empty + i, 3 + int(rng.integers(0, 2))))
    for i in range(n_one):
        rows.append(near(n_one + n_empty + n_few + i, 1))

    def pred(p, c):
        lens, blen, bor = _row_lens(c), _block_lens(c), p["borders"]
        capped = any(blen[b] == MAX_ROWS and p["blocks"][b][0] == MAX_ROWS for b in range(p["nblk"]))
        empty = any(blen[b] == MAX_ROWS and p["blocks"][b][0] == 0 for b in range(p["nblk"]))
        second_trip = any(blen[b] > LANES and lens[bor[b]:bor[b + 1]].min() >= 3 and lens[bor[b]:bor[b + 1]].max() <= 4
                          for b in range(p["nblk"]))
        offsets = np.unique(c.A.indices - np.repeat(np.arange(c.A.shape[0]), lens))
        return capped and empty and second_trip and offsets.size > 32 and p["window_on"] and c.long_rows.size == 0

    return Case("many_short_rows", T, _assemble(rows, n, rng, cplx),
                "a block that ends at the cap of 1024 rows, a block of 1024 empty rows, a block of more than 256 rows of three "
                "or four entries (a second trip of the row loop); more than 32 diagonals (not banded), inside a window operator",
                pred)


def rect_tail(T):
    rng = np.random.default_rng(17 + T)
    n_rows = 12 * T // 8
    n_cols = n_rows + 3000
    rows = [r for r in _band_rows(rng, n_rows, n_cols, shift=1500)]
    rows[-1] = rows[-1].copy()
    rows[-1][-1] = n_cols - 1
    return Case("rect_tail", T, _assemble(rows, n_cols, rng),
                "n_cols = n_rows + 3000 and the window of the last block ends exactly at column n_cols - 1",
                lambda p, c: c.A.shape[1] == c.A.shape[0] + 3000 and p["window_on"] and p["fit"] == p["nblk"] and
                p["blocks"][-1][1] + p["blocks"][-1][2] == c.A.shape[1] and p["blocks"][-1][3])


def banded_on_stream(T):
    nx, ny = 97, 53
    Tx = sp.diags([-np.ones(nx - 1), 2 * np.ones(nx), -np.ones(nx - 1)], [-1, 0, 1])
    Ty = sp.diags([-np.ones(ny - 1), 2 * np.ones(ny), -np.ones(ny - 1)], [-1, 0, 1])
    A = (sp.kron(Tx, sp.identity(ny)) + sp.kron(sp.identity(nx), Ty)).tocsr()
    A.sort_indices()
    return Case("banded_on_stream", T, A,
                "the 97 x 53 five-point Laplacian with the banded kernel switched off: the stream kernel, with the window, on "
                "the operator every benchmark uses",
                lambda p, c: p["window_on"] and p["fit"] == p["nblk"] and p["nblk"] > 1 and c.A.shape == (5141, 5141),
                switches={"spmv_dia": 0})


REAL = dict((f.__name__, f) for f in (all_fit, nine_of_ten, below_nine_of_ten, span_4096, span_4097, full_row_win,
                                      full_row_nowin, many_short_rows, rect_tail, banded_on_stream))
COMPLEX = dict((f.__name__, f) for f in (all_fit, full_row_win, full_row_nowin, many_short_rows))


@functools.lru_cache(maxsize=None)
def case(name, T):
    """The named real structure at tile ``T`` (built once per process; nobody may change it)."""
    return REAL[name](T)


@functools.lru_cache(maxsize=None)
def zcase(name, T):
    """The complex twin: the same pattern with complex values."""
    return COMPLEX[name](T, True)


def vector(n, ncols, seed, cplx=False):
    """``(n, ncols)`` operands with magnitudes in [1, 2) and random signs, Fortran-ordered."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(csigned(rng, (n, ncols)) if cplx else signed(rng, (n, ncols)))
