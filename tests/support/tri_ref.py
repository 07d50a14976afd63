"""Oracle of the sparse triangular solves - TEST INFRASTRUCTURE ONLY, shares no code with the package.

``tri_solve_ref`` is the plain sequential substitution, row by row:  ``s = b_i``;  ``s = s - t_ij * x_j`` over the off-diagonal
entries of row ``i`` in ascending column order;  ``x_i = s / t_ii`` (``x_i = s`` for a unit diagonal, a stored diagonal is then
ignored).  All arithmetic is done on NumPy scalars (``float64`` / ``complex128``), so a complex product and quotient round as
NumPy's do.  It is NOT ``scipy.sparse.linalg.spsolve_triangular``, which scales the rows first and differs in the last bits
when the diagonal is stored.

``levels_ref`` restates the level analysis (``level[i] = 1 + max level[j]`` over the off-diagonal entries) in NumPy."""
import numpy as np
import scipy.sparse as sp


def _canonical(T):
    T = sp.csr_matrix(T, copy=True)
    T.sum_duplicates()
    T.sort_indices()
    return T


def tri_solve_ref(T, b, lower, unit_diagonal=False):
    """``T^{-1} b`` for one vector or the columns of an ``(n, k)`` array; the result has the common type of T and b."""
    T = _canonical(T)
    b = np.asarray(b)
    dt = np.dtype(np.complex128) if (T.dtype.kind == "c" or b.dtype.kind == "c") else np.dtype(np.float64)
    n = T.shape[0]
    B = b.reshape(n, -1).astype(dt)
    X = np.zeros_like(B)
    indptr, indices, data = T.indptr, T.indices, T.data.astype(dt)
    rows = range(n) if lower else range(n - 1, -1, -1)
    for c in range(B.shape[1]):
        x, bb = X[:, c], B[:, c]
        for i in rows:
            s = bb[i]
            d = None
            for q in range(indptr[i], indptr[i + 1]):
                j = indices[q]
                if j == i:
                    d = data[q]
                else:
                    s = s - data[q] * x[j]
            if not unit_diagonal:
                s = s / d
            x[i] = s
    return X.reshape(b.shape) if b.ndim == 1 else X


def levels_ref(T, lower):
    """(level of every row counted from 1, rows per level) of the triangular matrix ``T``."""
    T = _canonical(T)
    n = T.shape[0]
    level = np.zeros(n, dtype=np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        cols = T.indices[T.indptr[i]: T.indptr[i + 1]]
        cols = cols[cols != i]
        level[i] = 1 + (level[cols].max() if cols.size else 0)
    return level, np.bincount(level)[1:]


def level_order_ref(T, lower):
    """Rows in the order of the device layout: by level, inside a level by (row length descending, row index ascending)."""
    T = _canonical(T)
    level, _ = levels_ref(T, lower)
    n = T.shape[0]
    length = np.diff(T.indptr) - (T.diagonal() != 0) - _stored_zero_diagonals(T)
    return np.lexsort((np.arange(n), -length, level))


def _stored_zero_diagonals(T):
    C = T.tocoo()
    z = np.zeros(T.shape[0], dtype=np.int64)
    hit = (C.row == C.col) & (C.data == 0)
    np.add.at(z, C.row[hit], 1)
    return z
