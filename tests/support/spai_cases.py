"""Matrices of the sparse-approximate-inverse tests (tests/test_spai_host.py, tests/test_gpu_spai.py) - TEST INFRASTRUCTURE ONLY.
``oracle(name)`` computes a case once, shares it and hands it out read-only."""
import functools

import numpy as np
import scipy.sparse as sp

from tests.support import tri_cases as tc
from tests.support.spai_ref import pattern_of, spai_ref


def _csr(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def convection_x(nx, ny, c=0.4):
    """Five-point Laplacian plus first-order upwind convection of strength ``c`` in x (point (ix, iy) has index ix * ny + iy):
    + c on the diagonal, - c towards ix - 1.  Unsymmetric M-matrix."""
    n = nx * ny
    return _csr(tc.lap2d(nx, ny) + c * sp.identity(n) - c * sp.diags(np.ones(n - ny), -ny, shape=(n, n)))


def complex_shifted(nx=12, ny=9):
    """The convection operator with a complex shift and seeded complex off-diagonal values; real-valued entries (imaginary part
    +0) stay among them."""
    rng = np.random.default_rng(21)
    A = sp.csr_matrix(convection_x(nx, ny, 0.3), dtype=np.complex128)
    f = 1.0 + 0.25j * rng.standard_normal(A.nnz)
    f[::3] = 1.0
    A.data = A.data * f
    return _csr(A + (0.4 + 0.7j) * sp.identity(nx * ny))


def make_complex(A, seed):
    rng = np.random.default_rng(seed)
    Z = sp.csr_matrix(A, dtype=np.complex128, copy=True)
    Z.data = Z.data * (1.0 + 0.3j * rng.standard_normal(Z.nnz))
    return _csr(Z)


def random_rows(n, seed, per_row=6):
    """About ``per_row + 1`` entries per row (uniform in [-1, 1], unsymmetric pattern), diagonal = sum |row| + 1."""
    rng = np.random.default_rng(seed)
    if n == 1:
        return sp.csr_matrix(np.array([[2.5]]))
    k = min(per_row, n - 1)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=n * k)
    keep = rows != cols
    R = _csr(sp.csr_matrix((rng.uniform(-1.0, 1.0, keep.sum()), (rows[keep], cols[keep])), shape=(n, n)))
    return _csr(R + sp.diags(np.asarray(abs(R).sum(axis=1)).ravel() + 1.0))


def band(n, hw, seed):
    rng = np.random.default_rng(seed)
    D = rng.uniform(-1.0, 1.0, (n, n))
    i, j = np.indices((n, n))
    D[abs(i - j) > hw] = 0.0
    D[np.arange(n), np.arange(n)] = 2.0 * hw + 1.5
    return _csr(D)


def one_long_row():
    """(A, P): a band matrix and a tridiagonal pattern in which row 20 holds exactly 32 entries (columns 3 .. 34)."""
    A = band(40, 16, 8)
    P = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(40, 40)).tolil()
    P[20, :] = 0.0
    P[20, 3:35] = 1.0
    P = _csr(P)
    assert np.diff(P.indptr).max() == 32 and np.diff(P.indptr)[20] == 32
    return A, P


def without_rows_and_diagonal(A, empty_rows):
    """The pattern of A without its diagonal and without the rows ``empty_rows``."""
    C = sp.coo_matrix(A)
    keep = (C.row != C.col) & ~np.isin(C.row, empty_rows)
    return _csr(sp.csr_matrix((np.ones(keep.sum()), (C.row[keep], C.col[keep])), shape=A.shape))


def identical_rows():
    """Rows 3 and 4 of A are the same (real) row: every pattern row that selects both has the Gram matrix of two equal vectors,
    d = g - (g / g) * g = 0 EXACTLY.  With the tridiagonal pattern rows 3 and 4 break down; row 3 is reported."""
    A = band(12, 2, 5).tolil()
    A[4, :] = A[3, :]
    return _csr(A), _csr(sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(12, 12)))


def zero_row():
    """Row 9 of A is a STORED zero row: G_aa = 0 for it, d = 0 exactly, in the pattern rows 8, 9, 10."""
    A = band(12, 2, 6)
    A.data[A.indptr[9]: A.indptr[10]] = 0.0
    return A, _csr(sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(12, 12)))


def two_broken_rows():
    """Both of the above in one matrix (rows 3 = 4 and a zero row 9): the smaller row, 3, is reported."""
    A = band(12, 2, 7).tolil()
    A[4, :] = A[3, :]
    A = _csr(A)
    A.data[A.indptr[9]: A.indptr[10]] = 0.0
    return A, _csr(sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(12, 12)))


def _grid(which, cplx):
    A = {"lap": lambda: tc.lap2d(37, 23), "conv": lambda: convection_x(37, 23)}[which]()
    return make_complex(A, 17) if cplx else A


CASES = {
    "lap_A": lambda: (tc.lap2d(37, 23), None),
    "lap_A2": lambda: (tc.lap2d(37, 23), tc.lap2d(37, 23) ** 2),
    "conv_A": lambda: (convection_x(37, 23), None),
    "conv_A2": lambda: (convection_x(37, 23), convection_x(37, 23) ** 2),
    "shifted_A": lambda: (complex_shifted(), None),
    "shifted_A2": lambda: (complex_shifted(), complex_shifted() ** 2),
    "zconv_A": lambda: (_grid("conv", True), None),
    "zconv_A2": lambda: (_grid("conv", True), _grid("conv", True) ** 2),
    "random_20001": lambda: (random_rows(20001, 5), None),
    "zrandom_20001": lambda: (make_complex(random_rows(20001, 5), 4), None),
    "long_row": one_long_row,
    "zlong_row": lambda: (make_complex(one_long_row()[0], 2), one_long_row()[1]),
    "gaps": lambda: (convection_x(9, 7), without_rows_and_diagonal(convection_x(9, 7), [0, 30, 62])),
    "zgaps": lambda: (make_complex(convection_x(9, 7), 6), without_rows_and_diagonal(convection_x(9, 7), [0, 30, 62])),
    "identical_rows": identical_rows,
    "zero_row": zero_row,
    "zzero_row": lambda: (make_complex(zero_row()[0], 1), zero_row()[1]),
    "two_broken_rows": two_broken_rows,
}
for _n in (1, 2, 63, 64, 65, 257):
    CASES["random_%d" % _n] = functools.partial(lambda n: (random_rows(n, 100 + n), None), _n)
    CASES["zrandom_%d" % _n] = functools.partial(lambda n: (make_complex(random_rows(n, 100 + n), n), None), _n)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """``(A, P, M, first_broken_row)`` of a case: A canonical CSR, P the canonical pattern as a CSR matrix of ones, M the oracle's
    matrix on it.  Computed once; the arrays are read-only."""
    A, P = CASES[name]()
    A = _csr(A)
    P = pattern_of(A if P is None else P)
    M, bad = spai_ref(A, P)
    for X in (A, P, M):
        for arr in (X.data, X.indices, X.indptr):
            arr.setflags(write=False)
    return A, P, M, bad
