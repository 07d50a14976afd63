"""Matrices of the triangular-solve tests (tests/test_tri_host.py, tests/test_gpu_tri.py) - TEST INFRASTRUCTURE ONLY."""
import numpy as np
import scipy.sparse as sp


def lap2d(nx, ny, order="natural"):
    """Five-point Laplacian on an nx x ny grid (point (ix, iy) has index ix * ny + iy), optionally in red-black order
    (points with ix + iy even first, each colour in natural order)."""
    A = (sp.kron(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx)), sp.identity(ny))
         + sp.kron(sp.identity(nx), sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(ny, ny)))).tocsr()
    if order == "redblack":
        p = np.arange(nx * ny)
        red = ((p // ny + p % ny) % 2) == 0
        perm = np.concatenate([p[red], p[~red]])
        A = A[perm][:, perm].tocsr()
    A.sort_indices()
    return A


def triangle(A, lower, strict=False):
    T = (sp.tril(A, -1 if strict else 0) if lower else sp.triu(A, 1 if strict else 0)).tocsr()
    T.sort_indices()
    return T


def make_complex(T, seed):
    """The same structure with seeded complex values (the diagonal kept away from zero)."""
    rng = np.random.default_rng(seed)
    T = sp.csr_matrix(T, dtype=np.complex128, copy=True)
    T.data = T.data * (1.0 + 0.5 * rng.standard_normal(T.nnz)) + 0.7j * rng.standard_normal(T.nnz) * np.abs(T.data)
    return T


def random_triangular(n, density, seed, lower=True, diag=True):
    """Seeded random sparse triangle: off-diagonal entries uniform in [-1, 1] scaled by 1 / (entries of the row), a diagonal in
    [1, 2] (so that the solve stays well scaled over many levels)."""
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=density, random_state=rng, format="csr", data_rvs=lambda k: rng.uniform(-1.0, 1.0, k))
    T = (sp.tril(R, -1) if lower else sp.triu(R, 1)).tocsr()
    cnt = np.maximum(np.diff(T.indptr), 1)
    T = sp.diags(1.0 / cnt).dot(T).tocsr()
    if diag:
        T = (T + sp.diags(rng.uniform(1.0, 2.0, n))).tocsr()
    T.sort_indices()
    return T


def bidiagonal(n, lower=True):
    d = 2.0 + 0.25 * np.cos(np.arange(n))
    o = -1.0 + 0.125 * np.sin(np.arange(n - 1))
    T = sp.diags([o, d], [-1 if lower else 1, 0], shape=(n, n)).tocsr() if n > 1 else sp.csr_matrix(d.reshape(1, 1))
    T.sort_indices()
    return T


def long_row(n, lower=True, width=500, seed=11):
    """A bidiagonal matrix with every third off-diagonal dropped (rows without off-diagonal entries mixed in) and ONE row
    that has `width` entries."""
    rng = np.random.default_rng(seed)
    T = bidiagonal(n, lower).tolil()
    for i in range(3, n, 3):
        j = i - 1 if lower else i + 1
        if 0 <= j < n:
            T[i, j] = 0.0
    r = n - 7 if lower else 6
    cols = rng.choice(np.arange(0, r) if lower else np.arange(r + 1, n), size=width, replace=False)
    for c in cols:
        T[r, c] = rng.uniform(-1.0, 1.0) / width
    T = T.tocsr()
    T.eliminate_zeros()
    T.sort_indices()
    return T
