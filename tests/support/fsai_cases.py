"""Matrices of the factorized-sparse-approximate-inverse tests (tests/test_fsai_host.py, tests/test_gpu_fsai.py) - TEST
INFRASTRUCTURE ONLY.  ``oracle(name)`` computes a case once, shares it and hands it out read-only."""
import functools

import numpy as np
import scipy.sparse as sp

from tests.support import tri_cases as tc
from tests.support.fsai_ref import fsai_ref, lower_pattern


def _csr(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def grid(cplx=False, nx=37, ny=23):
    """The five-point Laplacian on an nx x ny grid; ``cplx``: the Hermitian case A + 0.5 I + 0.3i (K - K^T), K = triu(A, 1) -
    positive definite by diagonal dominance (row sums of |off-diagonal| <= 4 sqrt(1.09) < 4.5)."""
    A = tc.lap2d(nx, ny)
    if not cplx:
        return _csr(A)
    K = sp.triu(A, 1)
    return _csr(A + 0.5 * sp.identity(nx * ny) + 0.3j * (K - K.T))


def power_pattern(A, k):
    """The pattern of A^k (the lower triangle is taken by the caller / by utils.fsai)."""
    B = _csr(abs(A))
    R = B
    for _ in range(k - 1):
        R = R @ B
    return _csr(R)


def band(n, hw, seed, cplx=False):
    """A symmetric / Hermitian band of half-width ``hw`` with seeded off-diagonal values in [-1, 1] (and imaginary parts for
    ``cplx``) and the diagonal 2 sqrt(2) hw + 1.5: positive definite by diagonal dominance."""
    rng = np.random.default_rng(seed)
    D = rng.uniform(-1.0, 1.0, (n, n)) + (1j * rng.uniform(-1.0, 1.0, (n, n)) if cplx else 0.0)
    i, j = np.indices((n, n))
    D[(i <= j) | (i - j > hw)] = 0.0
    D = D + D.conj().T
    D[np.arange(n), np.arange(n)] = 2.0 * np.sqrt(2.0) * hw + 1.5
    return _csr(D)


def random_symmetric(n, seed, per_row=3, cplx=False):
    """A seeded random symmetric / Hermitian pattern (about ``per_row`` entries below the diagonal per row, as many above),
    values uniform in [-1, 1], diagonal = sum |row| + 1: positive definite by diagonal dominance."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, size=n * per_row)
    keep = cols < rows
    vals = rng.uniform(-1.0, 1.0, keep.sum()) + (1j * rng.uniform(-1.0, 1.0, keep.sum()) if cplx else 0.0)
    Lo = _csr(sp.csr_matrix((vals, (rows[keep], cols[keep])), shape=(n, n)))
    R = _csr(Lo + Lo.conj().T)
    return _csr(R + sp.diags(np.asarray(abs(R).sum(axis=1)).ravel() + 1.0))


def one_long_row(cplx=False):
    """(A, P): a band matrix of half-width 32 and a bidiagonal pattern in which row 35 holds exactly 32 entries (columns 4 .. 35)."""
    A = band(48, 32, 8, cplx)
    P = sp.diags([1.0, 1.0], [-1, 0], shape=(48, 48)).tolil()
    P[35, 4:36] = 1.0
    P = _csr(P)
    assert np.diff(P.indptr).max() == 32 and np.diff(P.indptr)[35] == 32
    return A, P


def diagonal_pattern(cplx=False):
    """(A, P): the grid matrix with the pattern of the identity - every row has q = 1, u = 1, d = A_ii."""
    return grid(cplx, 9, 7), sp.identity(63, format="csr")


def missing_diagonal(cplx=False):
    """The band matrix without a stored entry (5, 5): S_jj = +0 for it.  Row 5 has d = 0 - L v exactly 0 or below (its pivot
    is minus a sum of squares over positive pivots), so row 5 is the first to break down, whatever the rounding."""
    A = band(12, 2, 5, cplx).tolil()
    A[5, 5] = 0.0
    A = _csr(A.tocsr())
    A.eliminate_zeros()
    assert A[5, 5] == 0 and 5 not in A.indices[A.indptr[5]: A.indptr[6]]
    return _csr(A), None


def indefinite(cplx=False):
    """A - 3 I on a 9 x 7 grid: row 0 has d = 4 - 3 = 1 > 0 (exact), row 1 has d = 1 - (-1 / 1) * (-1) = 0 exactly (every value
    a small integer): the first breakdown is row 1, whatever the rounding.  The Hermitian case: (A + 0.5 I + ...) - 3.5 I with
    the off-diagonal (-1 - 0.3i): row 1 has d = 1 - |(-1 - 0.3i)|^2 < 0."""
    A = grid(cplx, 9, 7)
    return _csr(A - (3.5 if cplx else 3.0) * sp.identity(63)), None


CASES = {
    "diagonal": lambda: (sp.diags(np.linspace(0.5, 4.0, 9)).tocsr(), None),
    "zdiagonal": lambda: (sp.diags(np.linspace(0.5, 4.0, 9).astype(complex)).tocsr(), None),
    "q1": diagonal_pattern,
    "zq1": lambda: diagonal_pattern(True),
    "random_20001": lambda: (random_symmetric(20001, 5), None),
    "zrandom_20001": lambda: (random_symmetric(20001, 5, cplx=True), None),
    "long_row": one_long_row,
    "zlong_row": lambda: one_long_row(True),
    "missing_diagonal": missing_diagonal,
    "zmissing_diagonal": lambda: missing_diagonal(True),
    "indefinite": indefinite,
    "zindefinite": lambda: indefinite(True),
    # the zero pivot d_1 = 0 in the MIDDLE of row 2 (J = 0, 1, 2): L_21 = -1 / 0 = -inf, d_2 = 1 - (-inf) * (-inf * 0) = NaN
    "indefinite_A2": lambda: (indefinite()[0], power_pattern(indefinite()[0], 2)),
}
for _k in (1, 2, 3, 4):
    CASES["lap_A%d" % _k] = functools.partial(lambda k: (grid(), power_pattern(grid(), k)), _k)
    CASES["zlap_A%d" % _k] = functools.partial(lambda k: (grid(True), power_pattern(grid(True), k)), _k)
for _n in (1, 2, 3, 63, 64, 65, 257):
    CASES["band_%d" % _n] = functools.partial(lambda n: (band(n, 3, 100 + n), None), _n)
    CASES["zband_%d" % _n] = functools.partial(lambda n: (band(n, 3, 100 + n, True), None), _n)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """``(A, P, U, d, first_broken_row)`` of a case: A canonical CSR, P the canonical LOWER pattern as a CSR matrix of ones, U the
    oracle's unscaled rows on it, d the last pivots.  Computed once; the arrays are read-only."""
    A, P = CASES[name]()
    A = _csr(A)
    P = lower_pattern(A if P is None else P)
    U, d, bad = fsai_ref(A, P)
    for X in (A, P, U):
        for arr in (X.data, X.indices, X.indptr):
            arr.setflags(write=False)
    d.setflags(write=False)
    return A, P, U, d, bad
