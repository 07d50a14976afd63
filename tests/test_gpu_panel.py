"""GPU tests of the per-column layer - the kernels every fast path of the library is compared with bit for bit, and what runs
after a recovered chain timeout, beyond 14.68 M rows and for the x update of every solver: k_multidot, k_multiaxpy with its
T_NRM / T_NRM_DIAG tails, k_reduce_partials, k_waxpby, k_vdiv, k_scale_store, k_minres_update, k_cg_update (kernels.h), their
c128 twins (zpath.h) and the block plumbing (kh_vec_copy / get / set / zero_range / upload / download).

The catalogue - which width selects which edge of the host code's chunk plans - is tests/support/panel_cases.py, the references
are tests/support/panel_ref.py; tests/test_panel_host.py holds both on the CPU.

Bars.  Everything that is not summed has the BITS of the order-exact NumPy fold.  Everything that is summed lies within
gamma(c) * sum|terms| of the longdouble value, c the longest chain of additions the kernel forms at that n and grid
(panel_ref.chain_*: derived from the code, not fitted).  Every output block is one column wider on each side than what is
written; those guard columns are compared bitwise and kh_vec_padding_nonzero is 0 after every sequence."""
import ctypes

import numpy as np
import pytest

from krypy_amd import _hip
from tests.support import panel_cases as pc
from tests.support import panel_ref as pr
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

LD = pr.LD
NAN = float("nan")


# ---- the context, tuned ------------------------------------------------------------------------------------------------------
@pytest.fixture
def tuned(hip):
    """``tuned(B)`` sets reduce_blocks to B (0: the default stays) and returns (context, the grid bound in force); the grid and
    every switch a test moved are put back afterwards."""
    nb0 = hip.info()["reduce_blocks"]
    before = {k: hip.get(k) for k in ("chain", "gram_mfma", "chain_onex")}

    def tune(reduce_blocks=0):
        if reduce_blocks:
            hip.tune(reduce_blocks=reduce_blocks)
        return hip, hip.info()["reduce_blocks"]

    try:
        yield tune
    finally:
        hip.tune(reduce_blocks=nb0)
        for k, v in before.items():
            if hip.get(k) != v:
                hip.set(k, v)


_CACHE = {}


def _cached(key, make):
    """a reference is computed once and shared by the grids (nobody writes to it)"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _clean(*blocks):
    for b in blocks:
        assert b.padding_nonzero() == 0, "a kernel wrote into the padding of a %d x %d block" % (b.n, b.ncols)


def _within(got, want, mag, c, what):
    """|got - want| <= gamma(c) sum|terms|, entry by entry; prints the worst ratio before it asserts"""
    err = np.abs(np.asarray(got, dtype=LD) - want).reshape(-1)
    bar = np.broadcast_to(pr.gamma(c) * np.asarray(mag, dtype=LD), np.shape(got)).reshape(-1)
    assert err.size and np.all(bar > 0), what + ": nothing to compare"
    worst = int(np.argmax(err / bar))
    print("%s: c = %d, worst error / bar = %.3f" % (what, c, float(err[worst] / bar[worst])))
    assert np.all(err <= bar), "%s: entry %d off by %.3e, bar %.3e (c = %d)" % (what, worst, float(err[worst]), float(bar[worst]), c)


def _bits(got, want, what):
    bad = np.nonzero(np.atleast_1d(got != want))[0]
    assert bad.size == 0 and got.shape == want.shape, "%s: %d entries differ, first at %d" % (what, bad.size, bad[0] if bad.size else -1)


# ---- a. inner products: dot_panel, gemm_tn with one right-hand column, nrm2 ---------------------------------------------------------
NDATA = 49          # data columns of the narrow blocks (47 at offset 1 ends at column 47; flush offsets end at 48); w is column 49
ZNDATA = 19


def _real_dot_ref(n):
    def make():
        B = pc.block(n, NDATA + 1, seed=n)
        vals, mags = pr.dot_ld(B[:, :NDATA], B[:, NDATA])
        return B, vals, mags, pr.sumsq_ld(B[:, NDATA])[0]
    return _cached(("rdot", n), make)


def _c128_dot_ref(n):
    def make():
        B = pc.block(n, ZNDATA + 1, seed=n + 1, cplx=True)
        w = B[:, ZNDATA]
        return (B,) + pr.zdot_ld(B[:, :ZNDATA].real, B[:, :ZNDATA].imag, w.real, w.imag) + (pr.sumsq_ld(w.real)[0] + pr.sumsq_ld(w.imag)[0],)
    return _cached(("zdot", n), make)


@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", pc.ROWS)
def test_real_inner_products(tuned, n, grid):
    """k_multidot<16 / 8 / 4 / 2 / 1> + k_reduce_partials at every narrow width and two offsets, w a column of V's own block:
    `out_dev + done` of the second outer chunk (17 ... 47), a chunk of one column, the same bits on a second call; kh_gemm_tn
    with one column on the right is the same launches; kh_nrm2."""
    ctx, nb = tuned(grid)
    B, vals, mags, ww = _real_dot_ref(n)
    Bd = ctx.upload(B)
    c = pr.chain_dot(n, nb)
    for width in pc.narrow(pc.REAL_WIDTHS):
        for j0 in pc.offsets(width, NDATA):
            what = "dot_panel n=%d nb=%d width=%d j0=%d" % (n, nb, width, j0)
            got = ctx.dot_panel(Bd, j0, width, Bd, NDATA)
            _within(got, vals[j0:j0 + width], mags[j0:j0 + width], c, what)
            _bits(ctx.dot_panel(Bd, j0, width, Bd, NDATA), got, what + ": second call")
            G = ctx.gemm_tn(Bd, j0, width, Bd, NDATA, 1)
            _bits(G[:, 0], got, what + ": gemm_tn with one right-hand column")
    nrm = ctx.nrm2(Bd, NDATA)
    ref = np.sqrt(ww)
    assert abs(LD(nrm) - ref) <= pr.sqrt_bar(c) * ref and nrm == ctx.nrm2(Bd, NDATA), "nrm2 n=%d: %r against %r" % (n, nrm, ref)
    _bits(Bd.download(), B, "the block is only read")
    _clean(Bd)


@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", pc.ROWS)
def test_c128_inner_products(tuned, n, grid):
    """k_zmultidot<8 / 4 / 2 / 1>: conj(v) w (a lost conjugate flips the sign of half the terms), `out_dev + 2 * done`."""
    ctx, nb = tuned(grid)
    B, re, im, are, aim, ww = _c128_dot_ref(n)
    Bd = ctx.upload(B)
    c = pr.chain_zdot(n, nb)
    for width in pc.narrow(pc.C128_WIDTHS):
        for j0 in pc.offsets(width, ZNDATA):
            what = "complex dot_panel n=%d nb=%d width=%d j0=%d" % (n, nb, width, j0)
            got = ctx.dot_panel(Bd, j0, width, Bd, ZNDATA)
            _within(got.real, re[j0:j0 + width], are[j0:j0 + width], c, what + " re")
            _within(got.imag, im[j0:j0 + width], aim[j0:j0 + width], c, what + " im")
            _bits(ctx.dot_panel(Bd, j0, width, Bd, ZNDATA), got, what + ": second call")
            _bits(ctx.gemm_tn(Bd, j0, width, Bd, ZNDATA, 1)[:, 0], got, what + ": gemm_tn")
    nrm = ctx.nrm2(Bd, ZNDATA)
    ref = np.sqrt(ww)
    assert abs(LD(nrm) - ref) <= pr.sqrt_bar(pr.chain_dot(2 * n, nb)) * ref, "complex nrm2 n=%d: %r against %r" % (n, nrm, ref)
    _bits(Bd.download(), B, "the block is only read")
    _clean(Bd)


# ---- b. updates: axpy_panel ------------------------------------------------------------------------------------------------------
def _guarded(ctx, w, seed, cplx=False):
    """[guard | w | guard] on the host and on the device"""
    Wh = pc.block(w.shape[0], 3, seed, cplx)
    Wh[:, 1] = w
    return Wh, ctx.upload(Wh)


@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", pc.ROWS)
def test_real_updates(tuned, n, grid):
    """k_multiaxpy<C, T_NONE, 1> through kh_axpy_panel: `coef_dev + done`, later chunks on the updated w, the odd tail."""
    ctx, nb = tuned(grid)
    B = _real_dot_ref(n)[0]
    Bd = ctx.upload(B)
    w = B[:, NDATA]
    Wh, Wd = _guarded(ctx, w, n + 2)
    for width in pc.narrow(pc.REAL_WIDTHS):
        for j0 in pc.offsets(width, NDATA):
            h = pc.coefficients(width, 100 * width + j0)
            want = _cached(("rfold", n, width, j0), lambda: pr.fold_real(w, B[:, j0:j0 + width], h, 1.0, 1.0))
            Wd.upload(1, w)
            ctx.axpy_panel(Bd, j0, width, h, Wd, 1)
            got = Wd.download()
            what = "axpy_panel n=%d nb=%d width=%d j0=%d" % (n, nb, width, j0)
            _bits(got[:, 1], want, what)
            _bits(got[:, [0, 2]], Wh[:, [0, 2]], what + ": guard columns")
    # w in V's own block, right behind the panel
    h = pc.coefficients(17, 5)
    ctx.axpy_panel(Bd, NDATA - 17, 17, h, Bd, NDATA)
    got = Bd.download()
    _bits(got[:, NDATA], pr.fold_real(w, B[:, NDATA - 17:NDATA], h, 1.0, 1.0), "axpy_panel into a column of V's block")
    _bits(got[:, :NDATA], B[:, :NDATA], "the panel is only read")
    _clean(Bd, Wd)


@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", pc.ROWS)
def test_c128_updates(tuned, n, grid):
    """k_zmultiaxpy<C, false, 1> through kh_zaxpy_panel."""
    ctx, nb = tuned(grid)
    B = _c128_dot_ref(n)[0]
    Bd = ctx.upload(B)
    w = B[:, ZNDATA]
    Wh, Wd = _guarded(ctx, w, n + 3, cplx=True)
    for width in pc.narrow(pc.C128_WIDTHS):
        for j0 in pc.offsets(width, ZNDATA):
            h = pc.coefficients(width, 100 * width + j0, cplx=True)
            V = B[:, j0:j0 + width]
            wr, wi = _cached(("zfold", n, width, j0), lambda: pr.fold_c128(w.real, w.imag, V.real.copy(), V.imag.copy(), h.real, h.imag, 1.0, 1.0))
            Wd.upload(1, w)
            ctx.axpy_panel(Bd, j0, width, h, Wd, 1)
            got = Wd.download()
            what = "complex axpy_panel n=%d nb=%d width=%d j0=%d" % (n, nb, width, j0)
            _bits(got[:, 1].real, wr, what + " re")
            _bits(got[:, 1].imag, wi, what + " im")
            _bits(got[:, [0, 2]], Wh[:, [0, 2]], what + ": guard columns")
    _bits(Bd.download(), B, "the panel is only read")
    _clean(Bd, Wd)


# ---- c. the widths around the caps (511 ... 1025), at 257 rows ----------------------------------------------------------------------
@pytest.mark.parametrize("grid", pc.GRIDS)
def test_real_widths_around_the_cap(tuned, grid):
    """1023, 1024 (the coefficients fill SC_COEF ... SC_LS to the last double) and 1025 (the wrapper's second C call, of one
    column), products and updates; afterwards the scalars behind the region still serve (an Arnoldi-free check: 16 dots)."""
    ctx, nb = tuned(grid)
    n, widths = pc.WIDE_ROWS, pc.wide(pc.REAL_WIDTHS)
    nd = max(widths) + 1

    def make():
        B = pc.block(n, nd + 1, seed=77)
        return (B,) + pr.dot_ld(B[:, :nd], B[:, nd])
    B, vals, mags = _cached(("rwide",), make)
    Bd = ctx.upload(B)
    w = B[:, nd]
    Wh, Wd = _guarded(ctx, w, 78)
    c = pr.chain_dot(n, nb)
    for width in widths:
        for j0 in pc.offsets(width, nd):
            what = "n=%d nb=%d width=%d j0=%d" % (n, nb, width, j0)
            got = ctx.dot_panel(Bd, j0, width, Bd, nd)
            _within(got, vals[j0:j0 + width], mags[j0:j0 + width], c, "dot_panel " + what)
            _bits(ctx.dot_panel(Bd, j0, width, Bd, nd), got, "dot_panel " + what + ": second call")
            _bits(ctx.gemm_tn(Bd, j0, width, Bd, nd, 1)[:, 0], got, "gemm_tn " + what)
            h = pc.coefficients(width, width + j0)
            want = _cached(("rwfold", width, j0), lambda: pr.fold_real(w, B[:, j0:j0 + width], h, 1.0, 1.0))
            Wd.upload(1, w)
            ctx.axpy_panel(Bd, j0, width, h, Wd, 1)
            got = Wd.download()
            _bits(got[:, 1], want, "axpy_panel " + what)
            _bits(got[:, [0, 2]], Wh[:, [0, 2]], "axpy_panel " + what + ": guard columns")
    _within(ctx.dot_panel(Bd, 1, 16, Bd, nd), vals[1:17], mags[1:17], c, "16 columns after the cap")
    _bits(Bd.download(), B, "the block is only read")
    _clean(Bd, Wd)


@pytest.mark.parametrize("grid", pc.GRIDS)
def test_c128_widths_around_the_cap(tuned, grid):
    """511, 512 (2 x 512 doubles fill the same region) and 513."""
    ctx, nb = tuned(grid)
    n, widths = pc.WIDE_ROWS, pc.wide(pc.C128_WIDTHS)
    nd = max(widths) + 1

    def make():
        B = pc.block(n, nd + 1, seed=79, cplx=True)
        return (B,) + pr.zdot_ld(B[:, :nd].real, B[:, :nd].imag, B[:, nd].real, B[:, nd].imag)
    B, re, im, are, aim = _cached(("zwide",), make)
    Bd = ctx.upload(B)
    w = B[:, nd]
    Wh, Wd = _guarded(ctx, w, 80, cplx=True)
    c = pr.chain_zdot(n, nb)
    for width in widths:
        for j0 in pc.offsets(width, nd):
            what = "complex n=%d nb=%d width=%d j0=%d" % (n, nb, width, j0)
            got = ctx.dot_panel(Bd, j0, width, Bd, nd)
            _within(got.real, re[j0:j0 + width], are[j0:j0 + width], c, "dot_panel re " + what)
            _within(got.imag, im[j0:j0 + width], aim[j0:j0 + width], c, "dot_panel im " + what)
            _bits(ctx.dot_panel(Bd, j0, width, Bd, nd), got, "dot_panel " + what + ": second call")
            _bits(ctx.gemm_tn(Bd, j0, width, Bd, nd, 1)[:, 0], got, "gemm_tn " + what)
            h = pc.coefficients(width, width + j0, cplx=True)
            V = B[:, j0:j0 + width]
            wr, wi = _cached(("zwfold", width, j0), lambda: pr.fold_c128(w.real, w.imag, V.real.copy(), V.imag.copy(), h.real, h.imag, 1.0, 1.0))
            Wd.upload(1, w)
            ctx.axpy_panel(Bd, j0, width, h, Wd, 1)
            got = Wd.download()
            _bits(got[:, 1].real, wr, "axpy_panel re " + what)
            _bits(got[:, 1].imag, wi, "axpy_panel im " + what)
            _bits(got[:, [0, 2]], Wh[:, [0, 2]], "axpy_panel " + what + ": guard columns")
    _bits(Bd.download(), B, "the block is only read")
    _clean(Bd, Wd)


# ---- d. gemm_nn, per-column form ---------------------------------------------------------------------------------------------------
def _y_start(Y0, nc, beta):
    """the output block as uploaded: [guard | nc columns | guard]; with beta == 0 the output columns are NaN (must not be read)"""
    Y = Y0.copy()
    if beta == 0.0:
        Y[:, 1:nc + 1] = NAN
    return Y


def _gemm_nn_check(ctx, X, Xd, k, nc, alpha, beta, seed, what):
    n = X.shape[0]
    C = pc.coefficients(k * nc, seed).reshape(k, nc)
    Y0 = pc.block(n, nc + 2, seed + 1)
    Ys = _y_start(Y0, nc, beta)
    Yd = ctx.upload(Ys)
    p0 = ctx.get("n_panel_gemm")
    ctx.gemm_nn(Xd, 1, k, C, alpha, beta, Yd, 1)
    moved = ctx.get("n_panel_gemm") - p0
    got = Yd.download()
    want = pr.gemm_nn_real(X[:, 1:k + 1], C, alpha, beta, Ys[:, 1:nc + 1])
    assert np.all(np.isfinite(got[:, 1:nc + 1])), what + ": not finite (beta == 0 must not read Y)"
    _bits(got[:, 1:nc + 1], want, what)
    _bits(got[:, [0, nc + 1]], Y0[:, [0, nc + 1]], what + ": guard columns")
    _clean(Yd)
    expect_kernel(moved == 0, what + ": took k_panel_gemm_mfma (%d passes)" % moved)


@pytest.mark.parametrize("k", pc.GEMM_K)
def test_gemm_nn_per_column(tuned, k):
    """kh_gemm_nn by k_multiaxpy: one output column, 17 and 20 (past k_panel_gemm_mfma), 2 and 16 with the matrix cores switched
    off; k = 0 (Y scaled, kh_waxpby in place), the KMAX = 1024 pass loop (the second and third pass start from 1, not beta),
    BETA == 0 on NaN and BETA == 2."""
    ctx, nb = tuned()
    n = pc.WIDE_ROWS
    X = _cached(("gemmX",), lambda: pc.block(n, max(pc.GEMM_K) + 2, seed=91))[:, :k + 2]
    Xd = ctx.upload(X)
    assert pc.k_edges(k, pr.KMAX)
    for nc in pc.GEMM_NC + pc.GEMM_NC_OFF:
        ctx.set("gram_mfma", 0 if nc in pc.GEMM_NC_OFF else 1)
        for alpha, beta in pc.GEMM_AB:
            _gemm_nn_check(ctx, X, Xd, k, nc, alpha, beta, 1000 * k + nc, "gemm_nn k=%d nc=%d alpha=%g beta=%g" % (k, nc, alpha, beta))
    _bits(Xd.download(), X, "X is only read")
    _clean(Xd)


@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", pc.ROWS)
def test_gemm_nn_beta_forms_at_every_row_count(tuned, n, grid):
    """k_multiaxpy<C, T_NONE, 0 / 1 / 2> with 16 + 2 + 1 columns: grid-stride trips and the odd tail of the BETA forms."""
    ctx, nb = tuned(grid)
    k = 19
    X = _real_dot_ref(n)[0][:, :k + 2]
    Xd = ctx.upload(X)
    for alpha, beta in pc.GEMM_AB:
        _gemm_nn_check(ctx, X, Xd, k, 1, alpha, beta, n + 7, "gemm_nn n=%d nb=%d alpha=%g beta=%g" % (n, nb, alpha, beta))
    _clean(Xd)


# ---- e. gemm_nn on the matrix cores ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", pc.MFMA_NC)
@pytest.mark.parametrize("k", pc.MFMA_K)
def test_gemm_nn_matrix_cores_beyond_three_passes(tuned, k, nc):
    """k_panel_gemm_mfma<2, 0 / 1 / 2> in 16, 17 (the last of one column) and 18 passes of 64 columns."""
    ctx, nb = tuned()
    ctx.set("gram_mfma", 1)
    n = pc.WIDE_ROWS
    X = _cached(("gemmX",), lambda: pc.block(n, max(pc.GEMM_K) + 2, seed=91))[:, :k + 2]
    Xd = ctx.upload(X)
    c = pr.chain_panel_gemm(k)
    for alpha, beta in ((1.0, 0.0), (-0.75, 1.0), (2.0, 0.5)):
        what = "gemm_nn on the matrix cores k=%d nc=%d alpha=%g beta=%g" % (k, nc, alpha, beta)
        C = pc.coefficients(k * nc, k + nc).reshape(k, nc)
        Y0 = pc.block(n, nc + 2, k + nc + 1)
        Ys = _y_start(Y0, nc, beta)
        Yd = ctx.upload(Ys)
        p0 = ctx.get("n_panel_gemm")
        ctx.gemm_nn(Xd, 1, k, C, alpha, beta, Yd, 1)
        moved = ctx.get("n_panel_gemm") - p0
        got = Yd.download()
        want, mag = pr.gemm_nn_ld(X[:, 1:k + 1], C, alpha, beta, Y0[:, 1:nc + 1])
        assert np.all(np.isfinite(got[:, 1:nc + 1])), what + ": not finite"
        _within(got[:, 1:nc + 1], want, mag, c, what)
        _bits(got[:, [0, nc + 1]], Y0[:, [0, nc + 1]], what + ": guard columns")
        _clean(Yd)
        expect_kernel(moved == len(pr.passes(k, pr.KP)), what + ": %d passes of k_panel_gemm_mfma" % moved)
    _clean(Xd)


# ---- f. gemm_nn, c128 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", pc.ZGEMM_K)
def test_gemm_nn_c128(tuned, k):
    """kh_zgemm_nn by k_zmultiaxpy<C, false, 0 / 1 / 2>: k = 0 scales Y by beta (it used to return with Y untouched unless beta
    was 0), 512 at the cap, 513 and 1025 through the wrapper's calls of 512 (the later ones with beta = 1).  alpha has
    power-of-two parts: the host's C * alpha is then exact in its products, the same number fused or not."""
    ctx, nb = tuned()
    n = pc.WIDE_ROWS
    X = _cached(("zgemmX",), lambda: pc.block(n, max(pc.ZGEMM_K) + 2, seed=93, cplx=True))[:, :k + 2]
    Xd = ctx.upload(X)
    alpha = 0.5 - 2.0j
    assert pc.k_edges(k, pr.ZCAP)
    for nc in (1, 3):
        for beta in pc.ZGEMM_BETA:
            what = "complex gemm_nn k=%d nc=%d beta=%g" % (k, nc, beta)
            C = pc.coefficients(k * nc, 10 * k + nc, cplx=True).reshape(k, nc)
            Y0 = pc.block(n, nc + 2, 10 * k + nc + 1, cplx=True)
            Ys = _y_start(Y0, nc, beta)
            Yd = ctx.upload(Ys)
            ctx.gemm_nn(Xd, 1, k, C, alpha, beta, Yd, 1)
            got = Yd.download()
            V = X[:, 1:k + 1]
            wr, wi = pr.gemm_nn_c128(V.real.copy(), V.imag.copy(), C, alpha, beta, Ys[:, 1:nc + 1].real.copy(), Ys[:, 1:nc + 1].imag.copy())
            assert np.all(np.isfinite(got[:, 1:nc + 1])), what + ": not finite"
            _bits(got[:, 1:nc + 1].real, wr, what + " re")
            _bits(got[:, 1:nc + 1].imag, wi, what + " im")
            _bits(got[:, [0, nc + 1]], Y0[:, [0, nc + 1]], what + ": guard columns")
            _clean(Yd)
    _bits(Xd.download(), X, "X is only read")
    _clean(Xd)


# ---- g. the fused tails and k_scale_store ------------------------------------------------------------------------------------------
# kh_arnoldi_step_begin with gs_mode = KH_GS_CGS reaches try_cgs_reg first; with the chain family switched off (kh_ctx_set
# "chain" 0) that declines and the step is dot_panel_dev, k_waxpby on the H column, multiaxpy_cols with the tail fused into its
# LAST chunk (T_NRM, or T_NRM_DIAG with a Jacobi diagonal) and k_scale_store<A_PART>.  zstep_enqueue: the same with zdot_dev,
# k_zacc, zaxpy_dev (NRM = true), k_reduce_partials and k_scale_store<A_SCAL> on the (re, im) view.
TAIL_ROWS = (256, 257, 4097)


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", TAIL_ROWS)
def test_fused_tails_real(tuned, n, grid, jacobi):
    ctx, nb = tuned(grid)
    ctx.set("chain", 0)
    for cols in pc.TAIL_COLS:
        k = cols - 1
        what = "tail n=%d nb=%d k+1=%d jacobi=%s" % (n, nb, cols, jacobi)
        V = pc.block(n, k + 3, seed=n + cols)                       # columns 0 .. k, k + 1 is written, k + 2 is a guard
        P = pc.block(n, k + 3, seed=n + cols + 1) if jacobi else None
        d = np.abs(pc.block(n, 1, seed=n + cols + 2)[:, 0])
        Wh = pc.block(n, 4 if jacobi else 3, seed=n + cols + 3)     # [guard | w | (mw) | guard]
        w = Wh[:, 1].copy()
        Vd, Wd = ctx.upload(V), ctx.upload(Wh)
        Pd = ctx.upload(P) if jacobi else None
        Md = ctx.diag(d) if jacobi else None
        c0 = ctx.counters()
        H = ctx.arnoldi_step(None, Md, Vd, Pd, Wd, 1, k, 0, 1, _hip.GS_CGS)
        expect_kernel(ctx.counters() == c0, what + ": a chain kernel took the step")
        # the H column: inner products with V
        vals, mags = pr.dot_ld(V[:, :cols], w)
        _within(H[:cols], vals, mags, pr.chain_dot(n, nb), what + ": H[0 .. k]")
        # w after the update: the fold with the coefficients the device used, over P with a preconditioner
        Bk = P if jacobi else V
        wn = pr.fold_real(w, Bk[:, :cols], H[:cols], 1.0, 1.0)
        gotW = Wd.download()
        _bits(gotW[:, 1], wn, what + ": w")
        mw = d * wn if jacobi else wn
        if jacobi:
            _bits(gotW[:, 2], mw, what + ": mw = d w")
        _bits(gotW[:, [0, -1]], Wh[:, [0, -1]], what + ": guard columns of W")
        s, _ = pr.sumsq_ld(wn, mw)
        h = H[k + 1]
        ref = np.sqrt(s)
        assert abs(LD(h) - ref) <= pr.sqrt_bar(pr.chain_dot(n, nb, extra=1 if jacobi else 0)) * ref, \
            what + ": H[k+1, k] = %r against %r" % (h, ref)
        # the next basis column(s): true division by the h the device returned
        gotV = Vd.download()
        _bits(gotV[:, k + 1], pr.vdiv(mw, h), what + ": v_{k+1}")
        keep = [j for j in range(k + 3) if j != k + 1]
        _bits(gotV[:, keep], V[:, keep], what + ": the basis and its guard column")
        if jacobi:
            gotP = Pd.download()
            _bits(gotP[:, k + 1], pr.vdiv(wn, h), what + ": p_{k+1}")
            _bits(gotP[:, keep], P[:, keep], what + ": P and its guard column")
            _clean(Pd)
        _clean(Vd, Wd)


@pytest.mark.parametrize("grid", pc.GRIDS)
@pytest.mark.parametrize("n", TAIL_ROWS)
def test_fused_tails_c128(tuned, n, grid):
    ctx, nb = tuned(grid)
    ctx.set("chain", 0)
    for cols in pc.TAIL_COLS:
        k = cols - 1
        what = "complex tail n=%d nb=%d k+1=%d" % (n, nb, cols)
        V = pc.block(n, k + 3, seed=n + cols + 5, cplx=True)
        Wh = pc.block(n, 3, seed=n + cols + 6, cplx=True)
        w = Wh[:, 1].copy()
        Vd, Wd = ctx.upload(V), ctx.upload(Wh)
        c0 = ctx.counters()
        H = ctx.arnoldi_step(None, None, Vd, None, Wd, 1, k, 0, 1, _hip.GS_CGS)
        expect_kernel(ctx.counters() == c0, what + ": a chain kernel took the step")
        re, im, are, aim = pr.zdot_ld(V[:, :cols].real, V[:, :cols].imag, w.real, w.imag)
        _within(H[:cols].real, re, are, pr.chain_zdot(n, nb), what + ": Re H[0 .. k]")
        _within(H[:cols].imag, im, aim, pr.chain_zdot(n, nb), what + ": Im H[0 .. k]")
        Vc = V[:, :cols]
        wr, wi = pr.fold_c128(w.real, w.imag, Vc.real.copy(), Vc.imag.copy(), H[:cols].real.copy(), H[:cols].imag.copy(), 1.0, 1.0)
        gotW = Wd.download()
        _bits(gotW[:, 1].real, wr, what + ": Re w")
        _bits(gotW[:, 1].imag, wi, what + ": Im w")
        _bits(gotW[:, [0, 2]], Wh[:, [0, 2]], what + ": guard columns of W")
        assert H[k + 1].imag == 0.0
        h = H[k + 1].real
        ref = np.sqrt(pr.sumsq_ld(wr)[0] + pr.sumsq_ld(wi)[0])
        assert abs(LD(h) - ref) <= pr.sqrt_bar(pr.chain_zdot(n, nb)) * ref, what + ": H[k+1, k] = %r against %r" % (h, ref)
        gotV = Vd.download()
        _bits(gotV[:, k + 1].real, pr.vdiv(wr, h), what + ": Re v_{k+1}")
        _bits(gotV[:, k + 1].imag, pr.vdiv(wi, h), what + ": Im v_{k+1}")
        keep = [j for j in range(k + 3) if j != k + 1]
        _bits(gotV[:, keep], V[:, keep], what + ": the basis and its guard column")
        _clean(Vd, Wd)


# ---- h. the streaming kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", pc.GRIDS)
def test_waxpby_vdiv_promote(tuned, grid):
    """k_waxpby at every special case of its coefficients (alpha == 1 and beta == 1 skip the multiply, beta == 0 does not read
    y), in the in-place form kh_gemm_nn's k == 0 branch uses (Z = X = Y); k_zwaxpby; k_vdiv, also in place (utils.py divides
    a reflector and the columns of a QR factor by their norms where they are); kh_zfrom_real."""
    ctx, nb = tuned(grid)
    for n in pc.ROWS:
        B = _real_dot_ref(n)[0][:, :5].copy()
        x, y = B[:, 1], B[:, 3]
        for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (1.0, 0.75), (-2.5, 0.0), (-2.5, 1.0), (-2.5, 0.75), (0.0, 0.0)):
            what = "waxpby n=%d nb=%d alpha=%g beta=%g" % (n, nb, alpha, beta)
            S = B.copy()
            if beta == 0.0:
                S[:, 3] = NAN
            Bd, Zd = ctx.upload(S), ctx.upload(B[:, :3])
            ctx.waxpby(Zd, 1, alpha, Bd, 1, beta, Bd, 3)
            got = Zd.download()
            _bits(got[:, 1], pr.waxpby(alpha, x, beta, y), what)
            _bits(got[:, [0, 2]], B[:, [0, 2]], what + ": guard columns")
            _clean(Zd, Bd)
        # in place: y = beta y as kh_gemm_nn(k == 0) asks for it, and z = alpha x + beta z
        Bd = ctx.upload(B)
        ctx.waxpby(Bd, 1, 0.5, Bd, 1, 0.0, Bd, 1)
        ctx.waxpby(Bd, 3, -2.5, Bd, 2, 0.75, Bd, 3)
        got = Bd.download()
        _bits(got[:, 1], pr.waxpby(0.5, x, 0.0, x), "waxpby in place, Z = X = Y, n=%d" % n)
        _bits(got[:, 3], pr.waxpby(-2.5, B[:, 2], 0.75, y), "waxpby in place, Z = Y, n=%d" % n)
        _bits(got[:, [0, 2, 4]], B[:, [0, 2, 4]], "waxpby in place: the other columns")
        # vdiv: out of place, in place
        ctx.vdiv(Bd, 4, Bd, 2, 1.7)
        ctx.vdiv(Bd, 2, Bd, 2, -3.3)
        got = Bd.download()
        _bits(got[:, 4], pr.vdiv(B[:, 2], 1.7), "vdiv n=%d" % n)
        _bits(got[:, 2], pr.vdiv(B[:, 2], -3.3), "vdiv in place n=%d" % n)
        _bits(got[:, 0], B[:, 0], "vdiv: column 0")
        _clean(Bd)
        # complex: zwaxpby, real coefficients on the (re, im) view, division by a complex scalar
        Z = _c128_dot_ref(n)[0][:, :5].copy()
        zx, zy = Z[:, 1], Z[:, 3]
        for a, b in ((0.5 + 0.25j, -1.5 + 2.0j), (1.0 + 0.0j, 0.0 + 1.0j), (0.5 - 0.25j, 0.0j)):
            what = "zwaxpby n=%d nb=%d alpha=%r beta=%r" % (n, nb, a, b)
            S = Z.copy()
            if b == 0:
                S[:, 3] = NAN
            Sd, Zd = ctx.upload(S), ctx.upload(Z[:, :3])
            ctx.waxpby(Zd, 1, a, Sd, 1, b, Sd, 3)
            got = Zd.download()
            rr, ri = pr.zwaxpby(a, zx.real, zx.imag, b, zy.real, zy.imag)
            _bits(got[:, 1].real, rr, what + " re")
            _bits(got[:, 1].imag, ri, what + " im")
            _bits(got[:, [0, 2]], Z[:, [0, 2]], what + ": guard columns")
            _clean(Zd, Sd)
        Zd = ctx.upload(Z)
        ctx.waxpby(Zd, 1, 0.5 + 0.25j, Zd, 1, -1.5 + 2.0j, Zd, 3)      # in place, Z = X
        ctx.waxpby(Zd, 2, -2.5, Zd, 2, 0.75, Zd, 3)                     # real coefficients: k_waxpby on the view, in place
        ctx.vdiv(Zd, 4, Zd, 0, 1.0 + 2.0j)                              # complex divisor: k_zwaxpby with 1 / s
        ctx.vdiv(Zd, 0, Zd, 0, 1.7)                                     # real divisor: k_vdiv on the view, in place
        got = Zd.download()
        rr, ri = pr.zwaxpby(0.5 + 0.25j, zx.real, zx.imag, -1.5 + 2.0j, zy.real, zy.imag)
        _bits(got[:, 1].real, rr, "zwaxpby in place re n=%d" % n)
        _bits(got[:, 1].imag, ri, "zwaxpby in place im n=%d" % n)
        _bits(got[:, 2].real, pr.waxpby(-2.5, Z[:, 2].real, 0.75, zy.real), "waxpby on a complex block re n=%d" % n)
        _bits(got[:, 2].imag, pr.waxpby(-2.5, Z[:, 2].imag, 0.75, zy.imag), "waxpby on a complex block im n=%d" % n)
        rr, ri = pr.zwaxpby(1.0 / complex(1.0 + 2.0j), Z[:, 0].real, Z[:, 0].imag, 0j, None, None)
        _bits(got[:, 4].real, rr, "vdiv by a complex scalar re n=%d" % n)
        _bits(got[:, 4].imag, ri, "vdiv by a complex scalar im n=%d" % n)
        _bits(got[:, 0].real, pr.vdiv(Z[:, 0].real, 1.7), "vdiv on a complex block, in place, re n=%d" % n)
        _bits(got[:, 0].imag, pr.vdiv(Z[:, 0].imag, 1.7), "vdiv on a complex block, in place, im n=%d" % n)
        _bits(got[:, 3], Z[:, 3], "column 3 is only read")
        _clean(Zd)
        # promote: columns 1 .. 2 of a real block into columns 2 .. 3 of a complex one
        Bd, Zd = ctx.upload(B), ctx.upload(Z)
        ctx.promote(Bd, 1, Zd, 2, 2)
        got = Zd.download()
        _bits(got[:, 2:4].real, B[:, 1:3], "promote re n=%d" % n)
        assert not got[:, 2:4].imag.any(), "promote im n=%d" % n
        _bits(got[:, [0, 1, 4]], Z[:, [0, 1, 4]], "promote: the columns around")
        _clean(Bd, Zd)


@pytest.mark.parametrize("grid", pc.GRIDS)
def test_minres_and_cg_updates(tuned, grid):
    """k_minres_update with either slot as W0; k_cg_update with and without a Jacobi diagonal: the vectors bit for bit, <r, z>
    within the bound of grid_lin's grid (up to 2 x reduce_blocks partials)."""
    ctx, nb = tuned(grid)
    for n in pc.ROWS:
        B = _real_dot_ref(n)[0]
        v, w0, w1, yk = B[:, 1], B[:, 2], B[:, 3], B[:, 4]
        r0, r1, r2, y0 = 0.625, -1.375, 1.75, 0.40625
        for slot in (0, 1):
            what = "minres_update n=%d nb=%d slot=%d" % (n, nb, slot)
            Wh = B[:, [2, 3, 5]] if slot == 0 else B[:, [3, 2, 5]]       # column `slot` holds W0; the third is a guard
            Vd, Wd, Yd = ctx.upload(B[:, :3]), ctx.upload(Wh), ctx.upload(B[:, 3:6])
            ctx.minres_update(Vd, 1, Wd, slot, r0, r1, r2, y0, Yd, 1)
            z, ynew = pr.minres_update(v, w0, w1, r0, r1, r2, y0, yk)
            gotW, gotY = Wd.download(), Yd.download()
            _bits(gotW[:, slot], z, what + ": z over W0")
            _bits(gotW[:, 1 - slot], w1, what + ": W1")
            _bits(gotW[:, 2], B[:, 5], what + ": guard column of W")
            _bits(gotY[:, 1], ynew, what + ": yk")
            _bits(gotY[:, [0, 2]], B[:, [3, 5]], what + ": guard columns of yk")
            _bits(Vd.download(), B[:, :3], what + ": V is only read")
            _clean(Vd, Wd, Yd)
        d = np.abs(B[:, 6])
        alpha = 0.40625
        for jacobi in (False, True):
            what = "cg_update n=%d nb=%d jacobi=%s" % (n, nb, jacobi)
            Pd, Yd, Rd = ctx.upload(B[:, 0:3]), ctx.upload(B[:, 3:6]), ctx.upload(B[:, 6:9])
            Ad, Zd = ctx.upload(B[:, 9:12]), ctx.upload(B[:, 12:15])
            Md = ctx.diag(d) if jacobi else None
            rho = ctx.cg_update(alpha, Pd, 1, Ad, 1, Yd, 1, Rd, 1, Md, Zd if jacobi else None, 1)
            ynew, rnew, znew = pr.cg_update(alpha, B[:, 1], B[:, 10], B[:, 4], B[:, 7], d if jacobi else None)
            gY, gR, gZ = Yd.download(), Rd.download(), Zd.download()
            _bits(gY[:, 1], ynew, what + ": yk")
            _bits(gR[:, 1], rnew, what + ": r")
            _bits(gZ[:, 1], znew if jacobi else B[:, 13], what + ": z")
            for g, lo in ((gY, 3), (gR, 6), (gZ, 12)):
                _bits(g[:, [0, 2]], B[:, [lo, lo + 2]], what + ": guard columns")
            s, mag = pr.sumsq_ld(rnew, znew)
            _within([rho], s, mag, pr.chain_cg(n, nb, jacobi), what + ": <r, z>")
            _clean(Pd, Yd, Rd, Ad, Zd)


# ---- i. the block plumbing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_block_plumbing(hip, n):
    ctx = hip
    B = pc.block(n, 8, seed=n + 40)
    # copy_from inside one block: overlapping ranges towards the front and towards the back, the same-column no-op
    Bd = ctx.upload(B)
    Bd.copy_from(1, Bd, 2, 4)
    want = B.copy()
    want[:, 1:5] = B[:, 2:6]
    _bits(Bd.download(), want, "copy_from, overlapping, towards the front")
    Bd.copy_from(3, Bd, 2, 4)
    want2 = want.copy()
    want2[:, 3:7] = want[:, 2:6]
    _bits(Bd.download(), want2, "copy_from, overlapping, towards the back")
    Bd.copy_from(2, Bd, 2, 3)
    _bits(Bd.download(), want2, "copy_from onto itself")
    _clean(Bd)
    # several columns between two blocks, one column, disjoint ranges of one block
    Sd, Dd = ctx.upload(B), ctx.upload(-B)
    Dd.copy_from(2, Sd, 4, 3)
    Dd.copy_from(6, Sd, 0, 1)
    want = -B
    want[:, 2:5] = B[:, 4:7]
    want[:, 6] = B[:, 0]
    _bits(Dd.download(), want, "copy_from between blocks")
    Sd.copy_from(0, Sd, 5, 2)
    want = B.copy()
    want[:, 0:2] = B[:, 5:7]
    _bits(Sd.download(), want, "copy_from, disjoint ranges of one block")
    _clean(Sd, Dd)
    # get / set / zero_range at the first element, with nothing, at the last element
    Bd = ctx.upload(B)
    assert Bd.get(3, 0, 1)[0] == B[0, 3] and Bd.get(3, n - 1, 1)[0] == B[n - 1, 3] and Bd.get(3, 0, 0).size == 0
    _bits(Bd.get(7, 0, n), B[:, 7], "get of a whole column")
    Bd.set(3, 0, [])
    Bd.set(3, n - 1, [])
    Bd.zero_range(3, 0, 0)
    Bd.zero_range(3, n, 0)
    _bits(Bd.download(), B, "set / zero_range of nothing")
    want = B.copy()
    Bd.set(2, n - 1, [7.5])
    Bd.set(4, 0, [-7.5])
    Bd.zero_range(5, n - 1, 1)
    Bd.zero_range(6, 0, 1)
    want[n - 1, 2], want[0, 4], want[n - 1, 5], want[0, 6] = 7.5, -7.5, 0.0, 0.0
    _bits(Bd.download(), want, "set / zero_range of the first and the last element")
    Bd.zero(2, 2)
    want[:, 2:4] = 0.0
    _bits(Bd.download(), want, "kh_vec_zero on a window")
    Bd.zero(5, 0)
    _bits(Bd.download(), want, "kh_vec_zero of no column")
    _clean(Bd)
    # upload / download of column windows from / into a host array whose leading dimension is larger than n
    ld = n + 5
    host = np.asfortranarray(pc.block(ld, 3, seed=n + 41))
    Bd = ctx.upload(B)
    ptr = host.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert ctx._lib.kh_vec_upload(Bd.handle, 4, 3, ptr, ld) == 0
    want = B.copy()
    want[:, 4:7] = host[:n]
    _bits(Bd.download(), want, "upload with host_ld > n")
    out = np.asfortranarray(np.full((ld, 2), 9.25))
    assert ctx._lib.kh_vec_download(Bd.handle, 5, 2, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ld) == 0
    _bits(out[:n], want[:, 5:7], "download with host_ld > n")
    assert np.all(out[n:] == 9.25), "download wrote behind row n of the host array"
    _bits(Bd.download(1, 2), want[:, 1:3], "download of a window")
    _clean(Bd)
    # the complex view: entries are (re, im) pairs
    Z = pc.block(n, 4, seed=n + 42, cplx=True)
    Zd = ctx.upload(Z)
    assert Zd.get(2, n - 1, 1)[0] == Z[n - 1, 2]
    Zd.set(1, n - 1, [1.5 - 2.5j])
    Zd.zero_range(3, 0, 1)
    Dd = ctx.alloc(n, 3, dtype=np.complex128)
    Dd.copy_from(1, Zd, 1, 1)
    want = Z.copy()
    want[n - 1, 1], want[0, 3] = 1.5 - 2.5j, 0.0
    _bits(Zd.download(), want, "set / zero_range on a complex block")
    got = Dd.download()
    _bits(got[:, 1], want[:, 1], "copy_from of a complex column")
    assert not got[:, [0, 2]].any()
    _clean(Zd, Dd)


def test_copy_of_one_column_between_blocks_padded_differently(tuned):
    """kh_vec_copy allows ONE column between blocks whose leading dimensions differ; padded_ld follows the public switch
    chain_onex, so two blocks of one length allocated on either side of kh_ctx_set can differ.  The copy moves the shorter of
    the two columns: with the source's (longer) one it wrote its zero padding over the head of the destination's NEXT column.
    The destination column is not the last of its block, so every byte touched lies inside the allocation either way."""
    ctx, nb = tuned()
    keep = ctx.get("chain_onex")
    try:
        found = None
        for n in (140000, 100000, 70000, 50000, 36000, 20000):
            ctx.set("chain_onex", 1)
            Sd = ctx.alloc(n, 2)
            ctx.set("chain_onex", 0)
            Dd = ctx.alloc(n, 3)
            if Sd.ld != Dd.ld:
                found = (n, Sd, Dd)
                break
        if found is None:
            pytest.skip("the leading dimensions are equal with and without chain_onex on %d compute units"
                        % ctx.info()["compute_units"])
        n, Sd, Dd = found
        print("n = %d: leading dimension %d with chain_onex, %d without" % (n, Sd.ld, Dd.ld))
        S, D = pc.block(n, 2, seed=51), pc.block(n, 3, seed=52)
        Sd.upload(0, S)
        Dd.upload(0, D)
        Dd.copy_from(0, Sd, 1, 1)          # the longer column into the shorter one's block (or the other way round)
        Sd.copy_from(0, Dd, 2, 1)          # ... and back
        want = D.copy()
        want[:, 0] = S[:, 1]
        _bits(Dd.download(), want, "destination: the column copied, the NEXT column untouched")
        wantS = S.copy()
        wantS[:, 0] = D[:, 2]
        _bits(Sd.download(), wantS, "the copy the other way round")
        _clean(Sd, Dd)
    finally:
        ctx.set("chain_onex", keep)
