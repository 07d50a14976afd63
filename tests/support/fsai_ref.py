"""Oracle of the factorized sparse approximate inverse on a fixed lower-triangular pattern - TEST INFRASTRUCTURE ONLY, shares no
code with the package.

``fsai_ref(A, P)`` restates the contract of krypy_amd/csrc/fsai.h as the plain sequential loop of one row, on NumPy ``float64``
values (a complex value is a pair of them, so that every rounding is spelled out: the product is ``(ac - bd, ad + bc)``, a complex
value times or over a real pivot is taken part by part).  As in tests/support/spai_ref.py the loop runs for all pattern rows of one
length AT ONCE - every variable is an array with one element per such row, every operation one NumPy ufunc call (one rounding per
element, nothing fused).  For row ``i`` with pattern columns ``J`` (ascending, ``J[-1] = i``):

    S_ab (a >= b) = the stored A[J_a, J_b] or +0 (bits copied; only the lower triangle of A is read)
    for j: v_k = L_jk * d_k (k < j);  d_j = Re(S_jj - sum_{k<j} L_jk conj(v_k));  L_ij = (S_ij - sum_{k<j} L_ik conj(v_k)) / d_j
    u_{q-1} = 1;  u_a = s, s = +0; s = s - L_ka * u_k   (k = a + 1 .. q - 1 ascending, a = q - 2 .. 0; L UNCONJUGATED)

The outputs are ``u`` at the pattern's CSR positions and ``d_i = d_{q-1}`` per row; row ``i`` of G is ``u / sqrt(d_i)``
(``fsai_matrix``).  The loop does NOT stop at a breakdown (a ``d_j`` that is not > 0 or not finite): it goes on and the smallest
row that broke down is reported.  A part that is a NaN is stored as the quiet NaN 0x7ff8000000000000 (infinities keep their
sign)."""
import numpy as np
import scipy.sparse as sp

from tests.support.spai_ref import ZERO, _canonical, _Complex, _Real, pattern_of


def lower_pattern(P):
    """``tril(P)`` with the diagonal added: the canonical CSR pattern (ones as values; stored zeros of P kept)."""
    P = pattern_of(P)
    n = P.shape[0]
    C = P.tocoo()
    keep = C.col <= C.row
    rows = np.concatenate([C.row[keep], np.arange(n)])
    cols = np.concatenate([C.col[keep], np.arange(n)])
    return pattern_of(sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=P.shape))


def _rows_ref(keys, Ar, Ai, n, J, cplx):
    """The rows with the ``q = J.shape[1]`` pattern columns ``J[r]``.  Returns (u: q pairs of arrays, d_last, broke)."""
    op = _Complex if cplx else _Real
    nr, q = J.shape
    S = {}
    for a in range(q):
        for b in range(a + 1):
            want = J[:, a] * n + J[:, b]
            pos = np.minimum(np.searchsorted(keys, want), keys.size - 1) if keys.size else np.zeros(nr, dtype=np.int64)
            hit = (keys[pos] == want) if keys.size else np.zeros(nr, dtype=bool)
            sr = np.where(hit, Ar[pos] if keys.size else 0.0, 0.0)
            si = np.where(hit, Ai[pos] if keys.size else 0.0, 0.0) if cplx else ZERO
            S[a, b] = (sr, si)
    L, d = {}, [None] * q
    broke = np.zeros(nr, dtype=bool)
    for j in range(q):
        v = [op.scale(L[j, k], d[k]) for k in range(j)]
        s = S[j, j]
        for k in range(j):
            s = op.sub(s, op.mul(L[j, k], op.conj(v[k])))
        d[j] = s[0]
        broke |= ~(d[j] > 0) | ~np.isfinite(d[j])
        for t in range(j + 1, q):
            s = S[t, j]
            for k in range(j):
                s = op.sub(s, op.mul(L[t, k], op.conj(v[k])))
            L[t, j] = op.over(s, d[j])
    u = [None] * q
    u[q - 1] = (np.ones(nr), np.zeros(nr) if cplx else ZERO)
    for a in range(q - 2, -1, -1):
        s = (np.zeros(nr), np.zeros(nr) if cplx else ZERO)
        for k in range(a + 1, q):
            s = op.sub(s, op.mul(L[k, a], u[k]))
        u[a] = s
    return u, d[q - 1], broke


def fsai_ref(A, P=None):
    """``(U, d, first_broken_row)``: U a CSR matrix on the lower pattern of ``P`` (None: of ``A``) with the unscaled rows ``u``
    (float64 / complex128), ``d`` the float64 vector of the last pivots."""
    A = _canonical(A)
    cplx = A.dtype.kind == "c"
    dt = np.dtype(np.complex128) if cplx else np.dtype(np.float64)
    A = A.astype(dt)
    if A.shape[0] != A.shape[1]:
        raise ValueError("a square matrix expected")
    P = lower_pattern(A if P is None else P)
    if P.shape != A.shape:
        raise ValueError("a pattern of the matrix's shape expected")
    n = A.shape[0]
    Ar = np.ascontiguousarray(A.data.real, dtype=np.float64)
    Ai = np.ascontiguousarray(A.data.imag, dtype=np.float64) if cplx else np.zeros(A.nnz)
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices          # ascending: A is canonical
    out_r, out_i, d = np.zeros(P.nnz), np.zeros(P.nnz), np.zeros(n)
    broke = np.zeros(n, dtype=bool)
    length = np.diff(P.indptr)
    with np.errstate(all="ignore"):
        for q in np.unique(length):
            rows = np.flatnonzero(length == q)
            at = P.indptr[rows].astype(np.int64)[:, None] + np.arange(q)
            u, dl, b = _rows_ref(keys, Ar, Ai, n, P.indices[at].astype(np.int64), cplx)
            broke[rows] = b
            d[rows] = dl
            for a in range(q):
                out_r[at[:, a]] = u[a][0]
                if cplx:
                    out_i[at[:, a]] = u[a][1]
    for arr in (out_r, out_i, d):
        arr[np.isnan(arr)] = np.nan          # stored as 0x7ff8000000000000
    out = out_r
    if cplx:          # (part by part: no arithmetic touches an inf or a NaN here)
        out = np.empty(P.nnz, dtype=np.complex128)
        out.real, out.imag = out_r, out_i
    U = sp.csr_matrix((out, P.indices.copy(), P.indptr.copy()), shape=A.shape)
    bad = int(np.flatnonzero(broke)[0]) if broke.any() else -1
    return U, d, bad


def scaled(U, d):
    """G: row i of U times ``1 / sqrt(d_i)`` - the host step of ``utils.fsai``, in the same NumPy operations."""
    scale = 1.0 / np.sqrt(d)
    return sp.csr_matrix((U.data * np.repeat(scale, np.diff(U.indptr)), U.indices.copy(), U.indptr.copy()), shape=U.shape)


def fsai_matrix(A, P=None):
    """The oracle's G (the breakdown-free case is asserted)."""
    U, d, bad = fsai_ref(A, P)
    assert bad == -1, bad
    return scaled(U, d)
