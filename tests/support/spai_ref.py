"""Oracle of the sparse approximate inverse on a fixed pattern - TEST INFRASTRUCTURE ONLY, shares no code with the package.

``spai_ref(A, P)`` restates the contract of krypy_amd/csrc/spai.h as the plain sequential loop of one row, on NumPy ``float64``
values (a complex value is a pair of them, so that every rounding is spelled out: the product is ``(ac - bd, ad + bc)``, a complex
value times or over a real pivot is taken part by part).  The loop runs for all pattern rows of one length AT ONCE - every
variable below is an array with one element per such row, every operation one NumPy ufunc call (one rounding per element, nothing
fused) - which changes no bit of any row and keeps an oracle for 20,000 rows within a second.  For row ``i`` with pattern columns
``J`` (ascending):

    G_ab (a >= b) = sum over the columns c both rows J_a, J_b hold, ascending, s = +0; s = s + conj(A[J_a, c]) * A[J_b, c]
    r_a = conj(A[J_a, i]) or 0
    for j: v_k = L_jk * d_k (k < j);  d_j = Re(G_jj - sum_{k<j} L_jk conj(v_k));  L_ij = (G_ij - sum_{k<j} L_ik conj(v_k)) / d_j
    y_a = r_a - sum_{k<a} L_ak y_k;  z_a = y_a / d_a;  m_a = z_a - sum_{k>a} conj(L_ka) m_k   (k ascending, a = q-1 .. 0)

The loop does NOT stop at a breakdown (a ``d_j`` that is not > 0 or not finite): it goes on - inf and NaN spread as IEEE arithmetic
spreads them - and the smallest row that broke down is reported.  IEEE 754 leaves the sign and payload of a NaN that an invalid
operation produces to the hardware, so the contract stores a part of ``m_a`` that is a NaN as the quiet NaN 0x7ff8000000000000
(infinities keep their sign)."""
import numpy as np
import scipy.sparse as sp

ZERO = np.float64(0.0)


def _canonical(A):
    A = sp.csr_matrix(A, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    return A


def pattern_of(P):
    """The canonical CSR pattern (ones as values; stored zeros kept) of a sparse or dense matrix."""
    if not sp.issparse(P):
        P = sp.csr_matrix(np.asarray(P) != 0)
    P = _canonical(P)
    return sp.csr_matrix((np.ones(P.nnz), P.indices, P.indptr), shape=P.shape)


class _Complex(object):
    """Pairs (re, im) of float64 arrays."""
    mul = staticmethod(lambda a, b: (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]))
    conj = staticmethod(lambda a: (a[0], -a[1]))
    sub = staticmethod(lambda a, b: (a[0] - b[0], a[1] - b[1]))
    add = staticmethod(lambda a, b: (a[0] + b[0], a[1] + b[1]))
    scale = staticmethod(lambda a, d: (a[0] * d, a[1] * d))
    over = staticmethod(lambda a, d: (a[0] / d, a[1] / d))


class _Real(object):
    """The same interface on real data: the second part is carried along as +0 and takes part in nothing."""
    mul = staticmethod(lambda a, b: (a[0] * b[0], ZERO))
    conj = staticmethod(lambda a: a)
    sub = staticmethod(lambda a, b: (a[0] - b[0], ZERO))
    add = staticmethod(lambda a, b: (a[0] + b[0], ZERO))
    scale = staticmethod(lambda a, d: (a[0] * d, ZERO))
    over = staticmethod(lambda a, d: (a[0] / d, ZERO))


def _rows_ref(A, Ar, Ai, J, rows, cplx):
    """The rows ``rows`` of M, all with ``q = J.shape[1]`` pattern columns ``J[r]``.  Returns (m: q pairs of arrays, broke: bool
    array, G: (len(rows), q, q) complex array, the Gram matrices)."""
    op = _Complex if cplx else _Real
    nr, q = J.shape
    ptr, idx = A.indptr.astype(np.int64), A.indices
    G = {}
    r = []
    for a in range(q):
        for b in range(a + 1):
            pa, ea = ptr[J[:, a]].copy(), ptr[J[:, a] + 1]
            pb, eb = ptr[J[:, b]].copy(), ptr[J[:, b] + 1]
            s = (np.zeros(nr), np.zeros(nr) if cplx else ZERO)
            while True:          # the two-pointer merge, one step of every row per pass
                act = np.flatnonzero((pa < ea) & (pb < eb))
                if act.size == 0:
                    break
                ca, cb = idx[pa[act]], idx[pb[act]]
                h = act[ca == cb]
                if h.size:
                    x = op.conj((Ar[pa[h]], Ai[pa[h]]))
                    t = op.add((s[0][h], s[1][h] if cplx else ZERO), op.mul(x, (Ar[pb[h]], Ai[pb[h]])))
                    s[0][h] = t[0]
                    if cplx:
                        s[1][h] = t[1]
                pa[act[ca <= cb]] += 1
                pb[act[cb <= ca]] += 1
            G[a, b] = s
        # r_a = conj(A[J_a, i]), +0 where row J_a has no entry in column i
        ra = (np.zeros(nr), np.zeros(nr) if cplx else ZERO)
        p, e = ptr[J[:, a]].copy(), ptr[J[:, a] + 1]
        while True:
            act = np.flatnonzero(p < e)
            if act.size == 0:
                break
            h = act[idx[p[act]] == rows[act]]
            if h.size:
                x = op.conj((Ar[p[h]], Ai[p[h]]))
                ra[0][h] = x[0]
                if cplx:
                    ra[1][h] = x[1]
            p[act] += 1
        r.append(ra)
    Gfull = np.zeros((nr, q, q), dtype=complex)
    for (a, b), s in G.items():
        Gfull[:, a, b] = s[0] + 1j * s[1]
        Gfull[:, b, a] = s[0] - 1j * s[1]
    L, d = {}, [None] * q
    broke = np.zeros(nr, dtype=bool)
    for j in range(q):
        v = [op.scale(L[j, k], d[k]) for k in range(j)]
        s = G[j, j]
        for k in range(j):
            s = op.sub(s, op.mul(L[j, k], op.conj(v[k])))
        d[j] = s[0]
        broke |= ~(d[j] > 0) | ~np.isfinite(d[j])
        for t in range(j + 1, q):
            s = G[t, j]
            for k in range(j):
                s = op.sub(s, op.mul(L[t, k], op.conj(v[k])))
            L[t, j] = op.over(s, d[j])
    y = [None] * q
    for a in range(q):
        s = r[a]
        for k in range(a):
            s = op.sub(s, op.mul(L[a, k], y[k]))
        y[a] = s
    m = [None] * q
    for a in range(q - 1, -1, -1):
        s = op.over(y[a], d[a])
        for k in range(a + 1, q):
            s = op.sub(s, op.mul(op.conj(L[k, a]), m[k]))
        m[a] = s
    return m, broke, Gfull


def spai_ref(A, P=None, want_gram=False):
    """``(M, first_broken_row)`` - M a CSR matrix on the canonical pattern of ``P`` (None: that of ``A``) with float64 /
    complex128 values; with ``want_gram`` also the list of the rows' Gram matrices."""
    A = _canonical(A)
    cplx = A.dtype.kind == "c"
    dt = np.dtype(np.complex128) if cplx else np.dtype(np.float64)
    A = A.astype(dt)
    P = pattern_of(A if P is None else P)
    if not P.shape == A.shape or A.shape[0] != A.shape[1]:
        raise ValueError("a square matrix and a pattern of its shape expected")
    n = A.shape[0]
    Ar = np.ascontiguousarray(A.data.real, dtype=np.float64)
    Ai = np.ascontiguousarray(A.data.imag, dtype=np.float64) if cplx else np.zeros(A.nnz)
    out_r, out_i = np.zeros(P.nnz), np.zeros(P.nnz)
    broke = np.zeros(n, dtype=bool)
    grams = [np.zeros((0, 0), dtype=complex)] * n
    length = np.diff(P.indptr)
    with np.errstate(all="ignore"):
        for q in np.unique(length):
            if q == 0:
                continue
            rows = np.flatnonzero(length == q)
            at = P.indptr[rows].astype(np.int64)[:, None] + np.arange(q)
            m, b, G = _rows_ref(A, Ar, Ai, P.indices[at].astype(np.int64), rows, cplx)
            broke[rows] = b
            for a in range(q):
                out_r[at[:, a]] = m[a][0]
                if cplx:
                    out_i[at[:, a]] = m[a][1]
            if want_gram:
                for k, i in enumerate(rows):
                    grams[i] = G[k]
    out_r[np.isnan(out_r)] = np.nan          # stored as 0x7ff8000000000000
    out_i[np.isnan(out_i)] = np.nan
    out = out_r
    if cplx:          # (part by part: no arithmetic touches an inf or a NaN here)
        out = np.empty(P.nnz, dtype=np.complex128)
        out.real, out.imag = out_r, out_i
    M = sp.csr_matrix((out, P.indices.copy(), P.indptr.copy()), shape=A.shape)
    bad = int(np.flatnonzero(broke)[0]) if broke.any() else -1
    return (M, bad, grams) if want_gram else (M, bad)
