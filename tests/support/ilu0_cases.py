"""Matrices of the ILU(0) tests (tests/test_ilu0_host.py, tests/test_gpu_ilu0.py) - TEST INFRASTRUCTURE ONLY.

Every matrix here keeps the factorisation far from a breakdown by construction: strictly diagonally dominant rows, or an
M-matrix (the Laplacian, also with an upwind convection term), for which ILU(0) exists and its pivots grow no smaller than
those of the exact factorisation."""
import numpy as np
import scipy.sparse as sp

from tests.support import tri_cases as tc


def random_dominant(n, seed, per_row=8):
    """About ``per_row`` entries per row (uniform in [-1, 1], unsymmetric pattern), diagonal = sum |row| + 1."""
    rng = np.random.default_rng(seed)
    if n == 1:
        return sp.csr_matrix(np.array([[2.5]]))
    k = min(per_row, n - 1)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=n * k)
    keep = rows != cols
    R = sp.csr_matrix((rng.uniform(-1.0, 1.0, keep.sum()), (rows[keep], cols[keep])), shape=(n, n))
    R.sum_duplicates()
    A = (R + sp.diags(np.asarray(abs(R).sum(axis=1)).ravel() + 1.0)).tocsr()
    A.sort_indices()
    return A


def convection(nx, ny, order="natural", wind=0.8):
    """Five-point Laplacian plus first-order upwind convection along the grid lines (index ix * ny + iy: the neighbours
    iy - 1 inside a line): -wind on the sub-diagonal inside a line, +wind on the diagonal.  Unsymmetric M-matrix."""
    n = nx * ny
    sub = np.full(n - 1, -wind)
    sub[np.arange(1, n) % ny == 0] = 0.0          # no coupling across the end of a grid line
    C = (sp.diags(sub, -1) + wind * sp.identity(n)).tocsr()
    C.eliminate_zeros()
    A = (tc.lap2d(nx, ny) + C).tocsr()
    if order == "redblack":
        p = redblack_permutation(nx, ny)
        A = A[p][:, p].tocsr()
    A.sort_indices()
    return A


def redblack_permutation(nx, ny):
    """The permutation of ``tri_cases.lap2d(nx, ny, "redblack")``: points with ix + iy even first, each colour in natural order."""
    p = np.arange(nx * ny)
    red = ((p // ny + p % ny) % 2) == 0
    return np.concatenate([p[red], p[~red]])


def nine_point(nx, ny):
    """Nine-point stencil (8 on the diagonal, -1 to the eight neighbours), diagonally dominant."""
    T = lambda m: sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(m, m))
    A = (-sp.kron(T(nx), T(ny)) + 9.0 * sp.identity(nx * ny)).tocsr()
    A.sort_indices()
    return A


def tridiagonal(n):
    d = 2.5 + 0.25 * np.cos(np.arange(n))
    A = sp.diags([-1.0 + 0.125 * np.sin(np.arange(n - 1)), d, -1.0 - 0.0625 * np.cos(np.arange(n - 1))], [-1, 0, 1], shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def long_row(n=2000, width=500, seed=11):
    """A tridiagonal matrix with every third sub-diagonal entry dropped (rows without lower entries mixed in) and ONE row with
    `width` entries left of the diagonal, its diagonal raised to keep the row dominant: the merge loop at its longest."""
    rng = np.random.default_rng(seed)
    A = tridiagonal(n).tolil()
    for i in range(3, n, 3):
        A[i, i - 1] = 0.0
    r = n - 7
    for c in rng.choice(np.arange(0, r - 1), size=width, replace=False):
        A[r, c] = rng.uniform(-1.0, 1.0)
    A[r, r] = width + 3.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def make_complex(A, seed):
    """The same structure with values x (1 + 0.2i g), g seeded normal, and + 0.5i on the diagonal."""
    rng = np.random.default_rng(seed)
    Z = sp.csr_matrix(A, dtype=np.complex128, copy=True)
    Z.data = Z.data * (1.0 + 0.2j * rng.standard_normal(Z.nnz))
    Z = (Z + 0.5j * sp.identity(A.shape[0])).tocsr()
    Z.sort_indices()
    return Z


def without(A, pairs):
    """A copy without the entries (i, j) of `pairs`; nothing else leaves the pattern."""
    C = sp.coo_matrix(A)
    n = A.shape[1]
    keep = ~np.isin(C.row.astype(np.int64) * n + C.col, [i * n + j for i, j in pairs])
    B = sp.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)
    B.sort_indices()
    return B


def with_values(A, entries):
    """A copy with the STORED entries (i, j) set to the given values: a zero written here stays in the pattern."""
    A = sp.csr_matrix(A, copy=True)
    for (i, j), v in entries.items():
        q = A.indptr[i] + np.flatnonzero(A.indices[A.indptr[i]: A.indptr[i + 1]] == j)
        assert q.size == 1, (i, j)
        A.data[q[0]] = v
    return A


def two_zero_pivots():
    """Two independent zero pivots in different levels.  Rows 14, 15 are [[1, 1], [1, 1]] cut off from rows 13 and 16: the pivot of
    row 15 is 1 - 1 * 1 = 0, in the second level.  Row 30 is cut off from row 29 and has a stored zero diagonal: a zero pivot in
    the FIRST level, so where every level is a launch of its own the larger row reports first.  The smaller row is 15."""
    A = without(tridiagonal(40), [(14, 13), (13, 14), (16, 15), (15, 16), (30, 29), (29, 30)])
    return with_values(A, {(14, 14): 1.0, (14, 15): 1.0, (15, 14): 1.0, (15, 15): 1.0, (30, 30): 0.0})


def strict_lower(A):
    return tc.triangle(A, True, strict=True)
