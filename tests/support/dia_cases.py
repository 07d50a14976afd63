"""Catalogue of the banded (diagonal-major) SpMV / SpMM tests - TEST INFRASTRUCTURE ONLY, imports nothing from the package
(tests/test_dia_host.py, tests/test_gpu_dia.py).

Two things live here.

(i) ``dia_plan``: a restatement of the host-side rule of ``kh_csr_upload`` / ``kh_zcsr_upload`` for the banded form
(``detect_dia`` and ``build_dia`` in krypy_amd/csrc/krylov_hip.hip).  An operator is banded when it is square with at least two
rows, has between 1 and 32 n stored entries, every row's columns ascend strictly, no stored value is zero (complex: both parts
zero), its entries sit on at most 32 distinct diagonals and those are at least 70 % full - ``not (float(nnz) < 0.7 * float(nd)
* float(n))``, the same double expression in the same order as the C++.  A real operator whose every diagonal holds ONE value
(bitwise) on at most 8 diagonals is kept as presence masks (``masked``), every other one as the value copy.  A complex operator
is taken only with 5 or 7 diagonals.  ``nd_template`` is the ND parameter of ``k_spmv_dia`` (3, 5, 7, 9, else 0 = the generic
loop), ``rows_per_wg = 512 * rpt`` and ``nblk`` the launch geometry for ``rpt`` row pairs per lane.

(ii) Named structures (``Case``), each with the property it exists for as text (``claim``) and as a predicate over ``dia_plan``
(``holds``): a structure that stops selecting what it claims fails on the CPU, before any kernel runs.  Values have magnitudes in
[1, 2) and random signs from a seeded generator; the constant variants hold one such value per diagonal.  The largest
structure has 18,431 rows.

The complex patterns at n = 7.  The offsets of the complex nd = 5 / nd = 7 / far7 patterns reach further than seven rows, so at
n = 7 the patterns themselves give 3 diagonals, 5 diagonals at 23 of 24.5 entries and 7 diagonals at 31 of 34.3 entries: all
three are NOT banded (``z5_7``, ``z7_7``, ``zfar7_7`` claim that).  The banded complex operators of seven rows are the contiguous
bands ``z5c_7`` (-2 .. 2) and ``z7c_7`` (-3 .. 3).

``k_zspmv_dia<0>`` (the generic loop of the complex kernel) cannot be reached from the API: ``kh_zcsr_upload`` keeps a
diagonal-major copy for 5 or 7 diagonals only.  No structure here tries to.
"""
import functools

import numpy as np
import scipy.sparse as sp

DIA_MAX = 32                   # distinct diagonals of the banded form
DIA_CMAX = 8                   # diagonals of the mask form
LANES = 256
U = 2.0 ** -53


def gamma(m):
    """``m u / (1 - m u)``: the relative error bound of a sum of ``m`` terms in ANY order."""
    return m * U / (1.0 - m * U)


# ---- the plan ---------------------------------------------------------------------------------------------------------
def dia_plan(A, rpt=4):
    """``dict(banded, offsets, nd, masked, nd_template, rpt, rows_per_wg, nblk)`` of a CSR matrix as it is stored (nothing is
    sorted, summed or pruned first).  ``offsets`` / ``nd`` are those of the pattern whenever the row scan finishes - also when
    the fill rule or the complex rule then turns the operator down -, ``()`` / 0 when the scan gives up."""
    assert sp.isspmatrix_csr(A)
    n, n_cols = A.shape
    indptr = np.asarray(A.indptr, dtype=np.int64)
    indices = np.asarray(A.indices, dtype=np.int64)
    data = np.asarray(A.data)
    cplx = data.dtype.kind == "c"
    nnz = int(data.size)
    rows_per_wg = 2 * LANES * rpt
    out = dict(banded=False, offsets=(), nd=0, masked=False, nd_template=0, rpt=rpt, rows_per_wg=rows_per_wg,
               nblk=(n + rows_per_wg - 1) // rows_per_wg)
    if n != n_cols or n < 2 or nnz == 0 or nnz > DIA_MAX * n:
        return out
    lens = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    first = np.zeros(nnz, dtype=bool)
    first[indptr[:-1][lens > 0]] = True
    if np.any(~first[1:] & (indices[1:] <= indices[:-1])):          # columns ascend strictly within a row
        return out
    if np.any(data == 0):                                           # a stored zero (complex: both parts zero; -0.0 counts)
        return out
    off = indices - rows
    offsets = np.unique(off)
    if offsets.size > DIA_MAX:
        return out
    nd = int(offsets.size)
    out["offsets"], out["nd"] = tuple(int(o) for o in offsets), nd
    if float(nnz) < 0.7 * float(nd) * float(n):
        return out
    if cplx:
        out["banded"] = nd in (5, 7)
    else:
        out["banded"] = True
        if nd <= DIA_CMAX:
            bits = np.ascontiguousarray(data, dtype=np.float64).view(np.uint64)
            out["masked"] = all(np.unique(bits[off == o]).size == 1 for o in offsets)
    if out["banded"]:
        out["nd_template"] = nd if nd in (3, 5, 7, 9) else 0
    return out


# ---- building blocks --------------------------------------------------------------------------------------------------
def signed(rng, shape):
    """Magnitudes in [1, 2), random signs."""
    return rng.uniform(1.0, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)


def csigned(rng, shape):
    """Complex numbers whose real and imaginary parts both have magnitudes in [1, 2) and random signs."""
    return signed(rng, shape) + 1j * signed(rng, shape)


def _csr(n, rows, cols, vals, n_cols=None):
    """CSR from triplets without duplicates: rows in order, columns ascending, nothing summed or dropped."""
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return sp.csr_matrix((vals, cols.astype(np.int32), indptr), shape=(n, n if n_cols is None else n_cols))


def band(n, offsets, seed, const=False, cplx=False, keep=None, n_cols=None):
    """The operator with entries on ``offsets``: fresh values per entry, or - ``const`` - one value per diagonal.  ``keep``:
    the number of entries that stay (the others are deleted at random, at least one per diagonal stays)."""
    rng = np.random.default_rng(seed)
    draw = csigned if cplx else signed
    m = n if n_cols is None else n_cols
    rows, cols, vals = [], [], []
    for o in offsets:
        i = np.arange(max(0, -o), min(n, m - o), dtype=np.int64)
        rows.append(i)
        cols.append(i + o)
        vals.append(np.full(i.size, draw(rng, 1)[0]) if const else draw(rng, i.size))
    starts = np.cumsum([0] + [r.size for r in rows])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    if keep is not None:
        stay = np.zeros(rows.size, dtype=bool)
        for d in range(len(offsets)):                               # every diagonal stays represented
            stay[rng.integers(starts[d], starts[d + 1])] = True
        rest = np.flatnonzero(~stay)
        stay[rng.choice(rest, size=keep - int(stay.sum()), replace=False)] = True
        rows, cols, vals = rows[stay], cols[stay], vals[stay]
    return _csr(n, rows, cols, vals, n_cols)


class Case(object):
    """One structure: the matrix, the property it exists for as text and as a predicate over ``dia_plan``."""

    def __init__(self, name, A, claim, predicate):
        self.name, self.A, self.claim, self._predicate = name, A, claim, predicate
        self.cplx = A.dtype.kind == "c"
        self.n = A.shape[0]

    @functools.lru_cache(maxsize=None)
    def plan(self, rpt=4):
        return dia_plan(self.A, rpt)

    def holds(self, plan=None):
        return bool(self._predicate(self.plan() if plan is None else plan, self))

    def __repr__(self):
        return self.name


def _value(nd):
    return lambda p, c: p["banded"] and not p["masked"] and p["nd"] == nd and p["nd_template"] == (nd if nd in (3, 5, 7, 9) else 0)


def _mask(nd):
    return lambda p, c: p["banded"] and p["masked"] and p["nd"] == nd and p["nd_template"] == (nd if nd in (3, 5, 7) else 0)


def _not_banded(p, c):
    return not p["banded"]


# ---- every count of diagonals, at n = 4099: three workgroups at RPT 4, odd n, a last row pair whose second row is padding ----
N0 = 4099
ND_OFFSETS = {
    1: (1,),                                            # no main diagonal
    2: (0, 17),
    3: (-1, 0, 1),
    4: (-1000, 0, 1, 1000),
    5: (-31, -2, 0, 1, 30),
    6: (-300, -2, -1, 0, 1, 300),
    7: (-9, -4, -1, 0, 2, 5, 8),
    8: (-64, -7, -2, -1, 0, 1, 6, 63),
    9: (-201, -200, -199, -1, 0, 1, 199, 200, 201),
    10: tuple(range(-5, 5)),
    16: tuple(range(-8, 8)),
    32: tuple(range(-16, 16)),
    33: tuple(range(-16, 17)),
}
ND_COUNTS = tuple(k for k in sorted(ND_OFFSETS) if k <= DIA_MAX)
ROW_EDGES = (3, 4, 5, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385, 18431)
FAR7 = lambda n: (-(n - 1), -2, -1, 0, 1, 2, n - 1)     # noqa: E731

_BUILD = {}


def _register(name, build):
    assert name not in _BUILD, name
    _BUILD[name] = build


def _register_band(name, n, offsets, seed, const, claim, predicate, cplx=False, keep=None):
    _register(name, lambda: Case(name, band(n, offsets, seed, const=const, cplx=cplx, keep=keep), claim, predicate))


for _nd in ND_COUNTS:
    _register_band("nd%d_value" % _nd, N0, ND_OFFSETS[_nd], 100 + _nd, False,
                   "%d diagonals with values of their own: the value copy, template ND = %d" % (_nd, _nd if _nd in (3, 5, 7, 9) else 0),
                   _value(_nd))
    if _nd <= DIA_CMAX:
        _register_band("nd%d_const" % _nd, N0, ND_OFFSETS[_nd], 200 + _nd, True,
                       "%d constant diagonals: the mask form" % _nd, _mask(_nd))
    else:
        _register_band("nd%d_const" % _nd, N0, ND_OFFSETS[_nd], 200 + _nd, True,
                       "%d constant diagonals are more than the mask form holds: banded, the value copy" % _nd, _value(_nd))
_register_band("nd33", N0, ND_OFFSETS[33], 133, False, "33 diagonals: not banded, the CSR kernel serves",
               lambda p, c: not p["banded"] and p["nd"] == 0)

for _name, _offs in (("all_even", (-4, -2, 0, 2, 6)), ("all_odd", (-3, -1, 1, 5))):
    _what = ("every x access can take the aligned 16-byte load" if _name == "all_even"
             else "no x access can take the aligned load, no main diagonal")
    _register_band(_name + "_value", N0, _offs, 300 + len(_offs), False, "offsets %r: %s (value copy)" % (_offs, _what),
                   _value(len(_offs)))
    _register_band(_name + "_const", N0, _offs, 310 + len(_offs), True, "offsets %r: %s (mask form)" % (_offs, _what),
                   _mask(len(_offs)))

_FAR7_CLAIM = ("n = 4099, offsets (-(n-1), -2, -1, 0, 1, 2, n-1): 20,491 entries against the bar of 20,085.1; two diagonals hold one "
               "entry each, nearly every row clamps at both ends")
_register_band("far7_value", N0, FAR7(N0), 320, False, _FAR7_CLAIM + " (value copy)",
               lambda p, c: _value(7)(p, c) and c.A.nnz == 20491 and p["offsets"] == FAR7(N0))
_register_band("far7_const", N0, FAR7(N0), 321, True, _FAR7_CLAIM + " (mask form)",
               lambda p, c: _mask(7)(p, c) and c.A.nnz == 20491 and p["offsets"] == FAR7(N0))


def _empty_rows(c):
    return int((np.diff(c.A.indptr) == 0).sum())


_register_band("threshold_in", 4100, (-2, -1, 0, 1, 2), 330, False,
               "n = 4100, five diagonals thinned to exactly 14,350 = 0.7 * 5 * 4100 entries: banded; some rows have no entry at all",
               lambda p, c: _value(5)(p, c) and c.A.nnz == 14350 and _empty_rows(c) >= 1, keep=14350)
_register_band("threshold_out", 4100, (-2, -1, 0, 1, 2), 330, False,
               "the same thinned to 14,349 entries, one below the bar: not banded; some rows have no entry at all",
               lambda p, c: not p["banded"] and p["nd"] == 5 and c.A.nnz == 14349 and _empty_rows(c) >= 1, keep=14349)


def _stored_zero():
    A = band(3001, (-1, 0, 1), 340)
    A.data[7] = 0.0
    return Case("stored_zero", A, "a tridiagonal operator with one stored zero: not banded", _not_banded)


def _unsorted_row():
    A = band(3001, (-1, 0, 1), 341)
    z = A.indptr[1500]
    A.indices[z], A.indices[z + 1] = A.indices[z + 1], A.indices[z]
    A.data[z], A.data[z + 1] = A.data[z + 1], A.data[z]
    return Case("unsorted_row", A, "a tridiagonal operator with the first two entries of row 1500 swapped: not banded",
                lambda p, c: not p["banded"] and not c.A.has_sorted_indices)


def _rectangular():
    A = band(3001, (-1, 0, 1), 342, n_cols=3002)
    return Case("rectangular", A, "3001 x 3002: not banded", lambda p, c: not p["banded"] and c.A.shape == (3001, 3002))


def _one_ulp():
    A = band(N0, ND_OFFSETS[8], 343, const=True)
    z = A.nnz // 3
    A.data[z] = np.nextafter(A.data[z], 0.0)
    return Case("one_ulp", A, "eight diagonals, constant but for ONE value moved by one ulp: banded, the value copy", _value(8))


_register("stored_zero", _stored_zero)
_register("unsorted_row", _unsorted_row)
_register("rectangular", _rectangular)
_register("one_ulp", _one_ulp)

for _n in ROW_EDGES:
    if _n == 3:         # 1 + 3 + 2 = 6 entries against the bar 0.7 * 3 * 3 = 6.3: the value pattern is banded from n = 4 on
        _register_band("edge3_value", 3, (-2, 0, 1), 403, False, "n = 3, offsets (-2, 0, 1): 6 entries below 6.3 - not banded",
                       lambda p, c: not p["banded"] and p["nd"] == 3 and c.A.nnz == 6)
    else:
        _register_band("edge%d_value" % _n, _n, (-2, 0, 1), 400 + _n, False,
                       "n = %d, offsets (-2, 0, 1) with values of their own: a border of the workgroups at 1, 2 or 4 row pairs per "
                       "lane" % _n, _value(3))
    _register_band("edge%d_const" % _n, _n, (-1, 0, 1), 500 + _n, True,
                   "n = %d, constant tridiagonal: the same border in the mask form" % _n, _mask(3))
_register_band("tri2", 2, (-1, 0, 1), 600, False, "tridiagonal at n = 2: 4 of 6 slots, 67 % full - not banded",
               lambda p, c: not p["banded"] and p["nd"] == 3 and c.A.nnz == 4)
_register_band("n2", 2, (0, 1), 601, False, "n = 2, offsets (0, 1): the smallest banded operator",
               lambda p, c: _value(2)(p, c) and c.A.nnz == 3)

REAL = tuple(_BUILD)

# ---- complex ------------------------------------------------------------------------------------------------------------
Z5, Z7 = ND_OFFSETS[5], ND_OFFSETS[7]


def _ztaken(nd):
    return lambda p, c: c.cplx and p["banded"] and p["nd"] == nd and p["nd_template"] == nd and not p["masked"]


for _n in (513, N0):
    _register_band("z5_%d" % _n, _n, Z5, 700 + _n, False, "complex, n = %d, five diagonals: k_zspmv_dia<5>" % _n, _ztaken(5), cplx=True)
    _register_band("z7_%d" % _n, _n, Z7, 710 + _n, False, "complex, n = %d, seven diagonals: k_zspmv_dia<7>" % _n, _ztaken(7), cplx=True)
    _register_band("zfar7_%d" % _n, _n, FAR7(_n), 720 + _n, False,
                   "complex far7 at n = %d: nearly every row clamps at both ends" % _n, _ztaken(7), cplx=True)
_register_band("z5_7", 7, Z5, 730, False, "complex, the five-diagonal pattern at n = 7 has three diagonals: not taken",
               lambda p, c: c.cplx and not p["banded"] and p["nd"] == 3, cplx=True)
_register_band("z7_7", 7, Z7, 731, False, "complex, the seven-diagonal pattern at n = 7: five diagonals, 23 entries below 24.5 - not taken",
               lambda p, c: c.cplx and not p["banded"] and p["nd"] == 5 and c.A.nnz == 23, cplx=True)
_register_band("zfar7_7", 7, FAR7(7), 732, False, "complex far7 at n = 7: 31 entries below 34.3 - not taken",
               lambda p, c: c.cplx and not p["banded"] and p["nd"] == 7 and c.A.nnz == 31, cplx=True)
_register_band("z5c_7", 7, (-2, -1, 0, 1, 2), 733, False, "complex, n = 7, offsets -2 .. 2: the smallest odd size k_zspmv_dia<5> serves",
               _ztaken(5), cplx=True)
_register_band("z7c_7", 7, (-3, -2, -1, 0, 1, 2, 3), 734, False, "complex, n = 7, offsets -3 .. 3: k_zspmv_dia<7>", _ztaken(7), cplx=True)
_register_band("z5_holes", N0, Z5, 740, False, "complex, five diagonals with 5 % of the entries deleted", _ztaken(5), cplx=True,
               keep=int(round(0.95 * sum(N0 - abs(o) for o in Z5))))
_register_band("z7_holes", N0, Z7, 741, False, "complex, seven diagonals with 5 % of the entries deleted", _ztaken(7), cplx=True,
               keep=int(round(0.95 * sum(N0 - abs(o) for o in Z7))))


def _z4():
    A = band(4, (-2, -1, 0, 1, 2), 750, cplx=True)
    z = A.indptr[2] + 1                      # an entry of row 2 becomes purely imaginary: (0, a) is no stored zero
    A.data[z] = 1j * A.data[z].imag
    return Case("z4", A, "complex, n = 4, offsets -2 .. 2: 14 entries exactly on the bar 0.7 * 5 * 4 - banded; one entry is (0, a)",
                lambda p, c: _ztaken(5)(p, c) and c.A.nnz == 14 and int(((c.A.data.real == 0) & (c.A.data.imag != 0)).sum()) == 1)


_register("z4", _z4)
_register_band("z3", 513, (-1, 0, 1), 760, False, "complex tridiagonal: full, but only 5 or 7 diagonals are taken",
               lambda p, c: c.cplx and not p["banded"] and p["nd"] == 3, cplx=True)
_register_band("z9", N0, ND_OFFSETS[9], 761, False, "complex, nine diagonals: full, but only 5 or 7 diagonals are taken",
               lambda p, c: c.cplx and not p["banded"] and p["nd"] == 9, cplx=True)

COMPLEX = tuple(k for k in _BUILD if k not in REAL)
ALL = REAL + COMPLEX


@functools.lru_cache(maxsize=None)
def case(name):
    """The named structure (built once per process; nobody may change it)."""
    return _BUILD[name]()


# ---- operands -----------------------------------------------------------------------------------------------------------
def vector(n, k, seed, cplx=False):
    """``(n, k)`` operands with magnitudes in [1, 2) and random signs, Fortran-ordered."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(csigned(rng, (n, k)) if cplx else signed(rng, (n, k)))


def edge_vector(A, seed=7):
    """``(x, rows)``: a vector of ``vector``'s kind with ``x[0] = +inf`` and ``x[n-1] = -inf`` (complex: in the real part), and
    the sorted rows that have an entry in column 0 or column n - 1 - the only rows whose product is not finite.  The banded
    kernels clamp the column of an empty slot to 0 or n - 1: the infinities sit exactly where a clamped load lands."""
    n = A.shape[1]
    x = vector(n, 1, seed, cplx=A.dtype.kind == "c")[:, 0].copy()
    x[0] = np.inf + (1j * x[0].imag if x.dtype.kind == "c" else 0.0)
    x[n - 1] = -np.inf + (1j * x[n - 1].imag if x.dtype.kind == "c" else 0.0)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    hit = (A.indices == 0) | (A.indices == n - 1)
    return x, np.unique(rows[hit])
