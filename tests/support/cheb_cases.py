"""Matrices of the Chebyshev preconditioner tests - TEST INFRASTRUCTURE ONLY (tests/test_cheb_host.py, tests/test_gpu_cheb.py,
tools/gen_cheb_golden.py, tools/cheb_bench.py)."""
import numpy as np
import scipy.sparse as sp


def lap1d(n, vary=False):
    """The three-point Laplacian; ``vary``: a diagonal 2 + i / n instead of 2 (no constant coefficients: the value form)."""
    d = 2.0 + (np.arange(n) / float(n) if vary else np.zeros(n))
    if n == 1:
        return sp.csr_matrix(np.array([[d[0]]]))
    A = sp.diags([-np.ones(n - 1), d, -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return A


def lap2d(nx, ny):
    """The five-point Laplacian on an nx x ny grid (Dirichlet), CSR with sorted indices."""
    Tx = sp.diags([-np.ones(nx - 1), 2 * np.ones(nx), -np.ones(nx - 1)], [-1, 0, 1])
    Ty = sp.diags([-np.ones(ny - 1), 2 * np.ones(ny), -np.ones(ny - 1)], [-1, 0, 1])
    A = (sp.kron(Tx, sp.identity(ny)) + sp.kron(sp.identity(nx), Ty)).tocsr()
    A.sort_indices()
    return A


def random_spd(n, per_row=7, seed=0):
    """A seeded random symmetric, strictly diagonally dominant matrix with about ``per_row`` entries per row at random places
    (no banded form: the CSR-stream kernel)."""
    rng = np.random.default_rng(seed)
    k = max((per_row - 1) // 2, 1)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=n * k)
    vals = rng.uniform(-1.0, 1.0, size=n * k)
    keep = rows != cols
    B = sp.coo_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    B = B + B.T
    diag = np.asarray(abs(B).sum(axis=1)).ravel() + 1.0 + rng.uniform(0.0, 1.0, size=n)
    A = (B + sp.diags(diag)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def gershgorin_lmax(A):
    return float(np.asarray(abs(sp.csr_matrix(A)).sum(axis=1)).max())


def hermitian_perturbed(nx, ny, seed=3, eps=0.05):
    """The five-point Laplacian plus a seeded Hermitian perturbation on its own pattern's off-diagonals, small enough to stay
    definite (the smallest eigenvalue of the 37 x 23 Laplacian is 0.024 and |perturbation| <= 4 * eps * 0.1)."""
    A = lap2d(nx, ny).tocoo()
    rng = np.random.default_rng(seed)
    up = A.row < A.col
    ph = 0.1 * eps * (rng.standard_normal(int(up.sum())) + 1j * rng.standard_normal(int(up.sum())))
    ph = ph / np.maximum(1.0, np.abs(ph) / (0.1 * eps))
    P = sp.coo_matrix((ph, (A.row[up], A.col[up])), shape=A.shape)
    H = (A.astype(complex) + P + P.conj().T).tocsr()
    H.sum_duplicates()
    H.sort_indices()
    return H
