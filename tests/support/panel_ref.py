"""References for the per-column layer of libkrylov_hip (kernels.h: k_multidot, k_multiaxpy and its tails, k_reduce_partials,
k_waxpby, k_vdiv, k_scale_store, k_minres_update, k_cg_update; zpath.h: k_zmultidot, k_zmultiaxpy, k_zwaxpby, kh_zgemm_nn,
kh_zfrom_real), written from the kernels' comments and shared with nothing: not with the library, not with
tests/support/numpy_context.py, not with the oracle.

Two kinds.

* ORDER-EXACT: float64 NumPy, one rounded operation per statement (NumPy fuses nothing; the library is compiled with
  -ffp-contract=off), in the order the kernel applies them.  The device result has these BITS.
* EXTENDED: everything that is summed (dots, norms, the fused tails, the matrix-core products) in ``np.longdouble``, returned
  with the sum of the absolute terms.  The device result lies within ``gamma(c) * sum|terms|`` of it, c being the longest chain
  of additions the kernel can form (the ``chain_*`` functions below derive it from the code).

The greedy chunk plans of the host code are restated here as plain functions (``split_real`` ...); tests/test_panel_host.py holds
them against brute force and reads the constants they assume out of the sources."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# what the sources say (tests/test_panel_host.py reads every one of them back out of the files)
MAXC, ZMAXC = 16, 8               # columns per k_multidot / k_multiaxpy launch, per k_zmultidot / k_zmultiaxpy launch
CAP, ZCAP = 1024, 512             # columns per C call: kh_dot_panel / kh_axpy_panel / kh_gemm_tn, their complex twins and kh_zgemm_nn
KMAX = 1024                       # coefficients per pass of kh_gemm_nn's per-column form
KP = 64                           # columns of X per pass of k_panel_gemm_mfma
BS = 256                          # lanes of a workgroup


def gamma(c):
    """gamma_c = c u / (1 - c u): the bound of c chained roundings."""
    return c * U / (1.0 - c * U)


# ---- split plans ------------------------------------------------------------------------------------------------------------
def _greedy(n, sizes):
    out = []
    while n > 0:
        c = next(s for s in sizes if n >= s)
        out.append(c)
        n -= c
    return out


def split_real(ncols):
    """The launches of multidot_chunk / multiaxpy_cols over ``ncols`` columns: 16 / 8 / 4 / 2 / 1, largest first."""
    return _greedy(ncols, (16, 8, 4, 2, 1))


def split_c128(ncols):
    """The launches of zdot_dev / zaxpy_dev: 8 / 4 / 2 / 1."""
    return _greedy(ncols, (8, 4, 2, 1))


def outer_chunks(ncols):
    """dot_panel_dev: runs of at most MAXC columns, each with its own reduction into ``out_dev + done``."""
    return [min(MAXC, ncols - d) for d in range(0, ncols, MAXC)]


def dot_launches_real(ncols):
    """Every k_multidot launch of dot_panel_dev as (first column, width)."""
    out, done = [], 0
    for nc in outer_chunks(ncols):
        d = 0
        for c in split_real(nc):
            out.append((done + d, c))
            d += c
        done += nc
    return out


def wrapper_calls(ncols, cap):
    """The C calls of the Python wrappers in _hip.py: strides of ``cap`` columns, left to right."""
    return [min(cap, ncols - d) for d in range(0, max(ncols, 1), cap)] if ncols > 0 else [0]


def passes(k, per_pass):
    return [min(per_pass, k - d) for d in range(0, k, per_pass)]


# ---- order-exact references: the folds -----------------------------------------------------------------------------------------
def _start(w, beta):
    """The three BETA forms of k_multiaxpy / k_zmultiaxpy: 1 keeps w, 0 starts from zero WITHOUT reading w, else beta * w."""
    if beta == 0.0:
        return np.zeros_like(w)
    if beta == 1.0:
        return w.copy()
    return beta * w


def fold_real(w, V, coef, sign, beta):
    """k_multiaxpy over the columns of V, left to right: h_c = sign * coef_c; w = w - h_c * v_c.  ``w`` may be (n,) with ``coef``
    (k,), or (n, m) with ``coef`` (k, m): m independent folds at once (elementwise, the same bits)."""
    w = _start(np.asarray(w, dtype=np.float64), beta)
    coef = np.asarray(coef, dtype=np.float64)
    for c in range(V.shape[1]):
        h = np.float64(sign) * coef[c]
        v = V[:, c] if w.ndim == 1 else V[:, c][:, None]
        t = h * v
        w = w - t
    return w


def fold_c128(wr, wi, Vr, Vi, cr, ci, sign, beta):
    """k_zmultiaxpy on separate (re, im) arrays: h = sign * coef; tr = hx vx - hy vy; ti = hx vy + hy vx; w -= (tr, ti)."""
    wr, wi = _start(np.asarray(wr, dtype=np.float64), beta), _start(np.asarray(wi, dtype=np.float64), beta)
    cr, ci = np.asarray(cr, dtype=np.float64), np.asarray(ci, dtype=np.float64)
    for c in range(Vr.shape[1]):
        hx = np.float64(sign) * cr[c]
        hy = np.float64(sign) * ci[c]
        vx = Vr[:, c] if wr.ndim == 1 else Vr[:, c][:, None]
        vy = Vi[:, c] if wr.ndim == 1 else Vi[:, c][:, None]
        a = hx * vx
        b = hy * vy
        tr = a - b
        a = hx * vy
        b = hy * vx
        ti = a + b
        wr = wr - tr
        wi = wi - ti
    return wr, wi


def gemm_nn_real(X, C, alpha, beta, Y):
    """kh_gemm_nn's per-column form, Y = beta Y + alpha X C: per output column coef = alpha * C[:, c], sign -1, passes of KMAX
    columns (the first with beta, the later ones keep Y).  k == 0: beta == 0 zeroes, beta == 1 leaves, else beta * Y (k_waxpby in
    place, its alpha * x with the add skipped)."""
    k = X.shape[1]
    Y = np.asarray(Y, dtype=np.float64)
    if k == 0:
        return _start(Y, beta)
    C = np.asarray(C, dtype=np.float64).reshape(k, -1)
    if Y.ndim == 1:
        C = C[:, 0]
    out, first = Y, True
    for i0 in range(0, k, KMAX):
        kk = min(KMAX, k - i0)
        coef = np.float64(alpha) * C[i0:i0 + kk]
        out = fold_real(out, X[:, i0:i0 + kk], coef, -1.0, beta if first else 1.0)
        first = False
    return out


def cmul(ar, ai, br, bi):
    """The device's complex product on (re, im): (ar br - ai bi, ar bi + ai br), every operation rounded."""
    p = ar * br
    q = ai * bi
    re = p - q
    p = ar * bi
    q = ai * br
    im = p + q
    return re, im


def gemm_nn_c128(Xr, Xi, C, alpha, beta, Yr, Yi):
    """Context.gemm_nn on complex blocks: C * alpha on the host (NumPy's complex product), kh_zgemm_nn in calls of ZCAP columns (the first
    with beta, the later ones with 1), each a fold with sign -1.  k == 0: the real entry's rule (beta is real)."""
    k = Xr.shape[1]
    Yr, Yi = np.asarray(Yr, dtype=np.float64), np.asarray(Yi, dtype=np.float64)
    if k == 0:
        return _start(Yr, beta), _start(Yi, beta)
    C = np.asarray(C, dtype=np.complex128).reshape(k, -1)
    if Yr.ndim == 1:
        C = C[:, 0]
    # (the one product taken from NumPy as it is: it happens on the HOST, inside Context.gemm_nn, and NumPy's complex loops
    # may contract it into fused multiply-adds where the CPU has them - cmul above would miss its last bit)
    Ca = np.asarray(C * alpha, dtype=np.complex128)
    Cr, Ci = Ca.real.copy(), Ca.imag.copy()
    first = True
    for i0 in range(0, k, ZCAP):
        kk = min(ZCAP, k - i0)
        Yr, Yi = fold_c128(Yr, Yi, Xr[:, i0:i0 + kk], Xi[:, i0:i0 + kk], Cr[i0:i0 + kk], Ci[i0:i0 + kk], -1.0,
                           beta if first else 1.0)
        first = False
    return Yr, Yi


# ---- order-exact references: the streaming kernels ------------------------------------------------------------------------------
def waxpby(alpha, x, beta, y):
    """k_waxpby: a = x if alpha == 1 else alpha * x; beta == 0 stores a (y is not read); b = y if beta == 1 else beta * y."""
    a = x.copy() if alpha == 1.0 else np.float64(alpha) * x
    if beta == 0.0:
        return a
    b = y if beta == 1.0 else np.float64(beta) * y
    return a + b


def zwaxpby(alpha, xr, xi, beta, yr, yi):
    """k_zwaxpby: r = alpha x (complex product, never skipped); beta == (0, 0) stores it; else r + beta y."""
    rr, ri = cmul(np.float64(alpha.real), np.float64(alpha.imag), xr, xi)
    if beta.real == 0.0 and beta.imag == 0.0:
        return rr, ri
    br, bi = cmul(np.float64(beta.real), np.float64(beta.imag), yr, yi)
    return rr + br, ri + bi


def vdiv(x, s):
    """k_vdiv and the store of k_scale_store: true division."""
    return x / np.float64(s)


def minres_update(v, w0, w1, r0, r1, r2, y0, yk):
    """k_minres_update: z = ((v - r0 w0) - r1 w1) / r2; yk + y0 z.  Returns (z, the new yk)."""
    t = np.float64(r0) * w0
    z = v - t
    t = np.float64(r1) * w1
    z = z - t
    z = z / np.float64(r2)
    t = np.float64(y0) * z
    return z, yk + t


def cg_update(alpha, p, ap, yk, r, d=None):
    """The vector part of k_cg_update: yk + alpha p; r - alpha Ap; z = d r (or r itself).  Returns (yk, r, z)."""
    t = np.float64(alpha) * p
    yk = yk + t
    t = np.float64(alpha) * ap
    r = r - t
    z = r if d is None else d * r
    return yk, r, z


# ---- extended precision --------------------------------------------------------------------------------------------------------
def dot_ld(V, w):
    """<v_j, w> for every column: (values, sums of |terms|) in longdouble."""
    t = np.asarray(V, dtype=LD) * np.asarray(w, dtype=LD)[:, None]
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def zdot_ld(Vr, Vi, wr, wi):
    """conj(v_j) w: (re, im, sum |terms of re|, sum |terms of im|).  re = vr wr + vi wi; im = vr wi - vi wr."""
    Vr, Vi = np.asarray(Vr, dtype=LD), np.asarray(Vi, dtype=LD)
    wr, wi = np.asarray(wr, dtype=LD)[:, None], np.asarray(wi, dtype=LD)[:, None]
    a, b, c, d = Vr * wr, Vi * wi, Vr * wi, Vi * wr
    return (a.sum(axis=0) + b.sum(axis=0), c.sum(axis=0) - d.sum(axis=0),
            np.abs(a).sum(axis=0) + np.abs(b).sum(axis=0), np.abs(c).sum(axis=0) + np.abs(d).sum(axis=0))


def sumsq_ld(w, m=None):
    """<w, m> (m = w by default) in longdouble; the terms of a norm are not negative when m = d w with d > 0."""
    t = np.asarray(w, dtype=LD) * np.asarray(w if m is None else m, dtype=LD)
    return t.sum(), np.abs(t).sum()


def gemm_tn_ld(X, Y):
    """X^T Y: (values, sums of |terms|)."""
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    return X.T.dot(Y), np.abs(X).T.dot(np.abs(Y))


def gemm_nn_ld(X, C, alpha, beta, Y):
    """beta Y + alpha X C with exact coefficients: (values, |beta Y| + |X| |alpha C|)."""
    X, Y = np.asarray(X, dtype=LD), np.asarray(Y, dtype=LD)
    aC = LD(alpha) * np.asarray(C, dtype=LD)
    if beta == 0.0:
        return X.dot(aC), np.abs(X).dot(np.abs(aC))
    return LD(beta) * Y + X.dot(aC), np.abs(LD(beta) * Y) + np.abs(X).dot(np.abs(aC))


# ---- the longest chain of additions --------------------------------------------------------------------------------------------
# A sum computed as a tree of rounded additions is within gamma(c) sum|terms| of the exact one, c being the largest number of
# additions any single term passes through.  The pieces, from kernels.h:
#   * a lane's serial loop: one fma per product (the product is not rounded, the accumulation is): `per_trip` roundings per trip
#     of the grid-stride loop, `trips` trips for the lane that makes the most;
#   * block_sum: wave_sum's shuffle tree, 6 additions (offsets 32 ... 1), then ((s0 + s1) + s2) + s3, 3 more: TREE = 9;
#   * the partials, one per workgroup, summed by ONE workgroup (k_reduce_partials, or bcast_sum_partials in the consumer's
#     prologue): a lane adds ceil(grid / 256) of them to 0.0, then block_sum again;
#   * + 1 for the reference itself: a longdouble product of two doubles is rounded to 64 bits and NumPy's pairwise longdouble
#     sum chains fewer than 64 additions even at 10^5 terms - together below 2^-58 sum|terms|, a small fraction of ONE u.
# Nothing here is fitted to a result.
TREE = 6 + 3


def grid_for(n, nb):
    """krylov_hip.hip: workgroups that cover n / 2 double2 elements, capped at the reduction grid."""
    return int(min(max(((n >> 1) + BS - 1) // BS, 1), nb))


def grid_lin(n, nb):
    return int(min(max((n + BS - 1) // BS, 1), 2 * nb))


def zgrid(n, nb):
    return int(min(max((n + BS - 1) // BS, 1), nb))


def _trips(items, grid):
    return -(-items // (grid * BS))


def _partials(grid):
    return -(-grid // BS) + TREE


def chain_dot(n, nb, extra=0):
    """k_multidot, k_gs_link<.., T_NRM> (kh_nrm2) and the T_NRM tail of k_multiaxpy: two fmas per double2 trip, one more in lane 0
    of workgroup 0 for an odd n, the tree, the partials.  ``extra``: roundings inside a term (T_NRM_DIAG rounds m = d w first)."""
    g = grid_for(n, nb)
    return 2 * _trips(n >> 1, g) + (n & 1) + TREE + _partials(g) + extra + 1


def chain_zdot(n, nb):
    """k_zmultidot and the NRM tail of k_zmultiaxpy over n complex entries: two fmas per accumulator and trip, no odd tail."""
    g = zgrid(n, nb)
    return 2 * _trips(n, g) + TREE + _partials(g) + 1


def chain_cg(n, nb, diag):
    """k_cg_update's <r, z>: one fma per trip on grid_lin's grid (up to 2 nb partials); z = d r is rounded first with a diagonal."""
    g = grid_lin(n, nb)
    return _trips(n, g) + TREE + _partials(g) + (1 if diag else 0) + 1


def chain_panel_gemm(k):
    """k_panel_gemm_mfma, one entry of Y: k accumulations on the matrix cores (k in place of the trip count: each 16x16x4
    instruction chains its four products onto the accumulator), one addition of the earlier value per pass of 64 columns, the
    rounding of beta * y, the rounding of alpha * C on the host, the reference."""
    return k + len(passes(k, KP)) + 3


def sqrt_bar(c):
    """relative bound of sqrt(|s|) for a sum s of non-negative terms within gamma(c): half of it, the root's own rounding, and
    half a u for the second-order terms (gamma(c)^2 < 1e-25 for every c used)."""
    return gamma(c + 1) / 2 + U
