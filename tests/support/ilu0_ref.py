"""Oracle of the ILU(0) factorisation - TEST INFRASTRUCTURE ONLY, shares no code with the package.

``ilu0_ref`` is the plain sequential loop on a copy ``a`` of the values of the canonical CSR matrix (sorted, duplicate-free,
stored zeros kept):

    for i = 0 .. n-1:
      for the entries p of row i with k = col[p] < i, ascending:
        a[p] = a[p] / a[dpos[k]]
        for the entries q of row i behind p, ascending: if (k, col[q]) is an entry r of row k: a[q] = a[q] - a[p] * a[r]

All arithmetic is done on NumPy scalars (``float64`` / ``complex128``): product and difference round separately, a complex
product and quotient round as NumPy's do.  The loop does NOT stop at a breakdown (a finished pivot that is zero or not finite): it
goes on - inf and NaN spread as IEEE arithmetic spreads them - and reports the smallest row that broke down."""
import numpy as np
import scipy.sparse as sp


def _canonical(A):
    A = sp.csr_matrix(A, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    return A


def split_factors(A, lu):
    """(L, U) as CSR from the factored values at the CSR positions of the canonical ``A``: L strictly lower plus explicit ones."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    out = []
    for mask in (A.indices <= rows, A.indices >= rows):
        data = lu[mask].copy()
        if len(out) == 0:
            data[A.indices[mask] == rows[mask]] = 1.0
        ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[mask], minlength=n))])
        out.append(sp.csr_matrix((data, A.indices[mask].copy(), ptr), shape=A.shape))
    return out[0], out[1]


def ilu0_ref(A):
    """``(L, U, lu_data, first_bad_row)``; ``first_bad_row`` is -1 without a breakdown.  Raises ValueError for a row without a
    structural diagonal."""
    A = _canonical(A)
    dt = np.dtype(np.complex128) if A.dtype.kind == "c" else np.dtype(np.float64)
    n = A.shape[0]
    indptr, indices = A.indptr.tolist(), A.indices.tolist()
    a = list(A.data.astype(dt))          # NumPy scalars
    dpos = [-1] * n
    where = []                           # per row: column -> position
    for i in range(n):
        w = {indices[q]: q for q in range(indptr[i], indptr[i + 1])}
        where.append(w)
        if i not in w:
            raise ValueError("row %d has no diagonal entry" % i)
        dpos[i] = w[i]
    bad = -1
    with np.errstate(all="ignore"):
        for i in range(n):
            end = indptr[i + 1]
            for p in range(indptr[i], dpos[i]):
                k = indices[p]
                l = a[p] / a[dpos[k]]
                a[p] = l
                wk = where[k]
                for q in range(p + 1, end):
                    r = wk.get(indices[q])
                    if r is not None:
                        a[q] = a[q] - l * a[r]
            d = a[dpos[i]]
            if bad < 0 and (d == 0 or not np.isfinite(d)):
                bad = i
    lu = np.array(a, dtype=dt) if n else np.zeros(0, dtype=dt)
    L, U = split_factors(A, lu)
    return L, U, lu, bad
