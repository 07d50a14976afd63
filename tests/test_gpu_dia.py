"""GPU tests of the banded (diagonal-major) SpMV / SpMM - k_spmv_dia, k_spmm_dia, k_dia_fill, k_dia_mask_fill, detect_dia /
build_dia, k_zspmv_dia, k_zdia_fill - at every diagonal count, in both storage forms and at every row edge.  The structures
and the restated upload plan: tests/support/dia_cases.py (held on the CPU by tests/test_dia_host.py).

Bars.  Every product is compared bit for bit with ``A.dot(x)`` (SciPy's csr_matvec, the library's contract) on ALL rows.  Every
run starts from a poisoned output block and ends with clean padding.  Every sum is held to ``gamma_m * sum |terms|`` against a
``longdouble`` sum of the device's own (bit-exact) vector entries, gamma_m = m u / (1 - m u), u = 2^-53: the bound of a sum of
m terms in ANY order (tests/test_gpu_csr_stream.py: _sum_bar).  A norm is compared on its square: n squares, the root and its
square again - gamma_(n+2).  Operand magnitudes lie in [1, 2): a lost or repeated term moves a sum by at least 1.

Which test runs which instantiation of ``k_spmv_dia<EPI, ND, RPT, HALO = false>`` (form: v = value copy, m = presence masks;
RPT 4 is the default of this process, RPT 1 and 2 are the two child processes of test_row_pairs_per_lane):

    EPI_NONE  ND 3, 5, 7    v, m   RPT 4: test_apply_one_column (nd3/5/7_value, _const, edge*, far7_*, all_even_*, threshold_in)
                                   RPT 1, 2: test_row_pairs_per_lane (the same structures)
    EPI_NONE  ND 9          v      test_apply_one_column[nd9_value, nd9_const]; RPT 1, 2: the children    (no mask form: nd > 8)
    EPI_NONE  ND 0          v      test_apply_one_column[nd1/2/4/6/8/10/16/32_value, nd10/16/32_const, one_ulp, all_odd_value, n2]
    EPI_NONE  ND 0          m      test_apply_one_column[nd1/2/4/6/8_const, all_odd_const]; RPT 1, 2: the children
    EPI_RES   every ND      v, m   test_residual (the same structures); RPT 1, 2: the children
    EPI_DOT   ND 3, 5, 7, 9, 0  v  test_arnoldi_first_coefficient, test_cg_step (nd3/5/7/9/4_value, edge*_value)      RPT 4 only
    EPI_DOT   ND 3, 5, 7, 0     m  the same tests (nd3/5/7/4_const, edge*_const)                                         RPT 4 only
    EPI_CHEB  ND 7, 9, 0    v      test_cheb_epilogue[nd1/4/7/9/16_value, nd9/16_const]; ND 3: edge2049_value; RPT 1, 2: children
    EPI_CHEB  ND 7, 0, 3    m      test_cheb_epilogue[nd1/4/7_const, edge2049_const]; RPT 1, 2: the children (whole catalogue)
    split launches (blk_lo / blk_skip / part_off)   test_split_launches: EPI_NONE and EPI_RES, ND 3, v and m, RPT 4
    k_spmm_dia<8>           v, m   test_spmm (2 ... 17 columns), test_clamped_values (three columns)
    k_zspmv_dia<5>, <7>            test_apply_one_column[z*], test_clamped_values_complex

No public entry reaches: ``k_zspmv_dia<0>`` (kh_zcsr_upload keeps a banded copy for 5 or 7 diagonals only); the scalar x loads
of an even offset with a misaligned ``x`` (``xal`` false: the columns of a block are always 16-byte aligned) and, for the same
reason, EPI_CHEB's row-by-row tail ``chal`` false; EPI_DOT at RPT 1 and 2 has entries (kh_arnoldi_step, kh_cg_step) but the
children leave it to the default mode; the HALO / XH forms belong to tests/test_gpu_halo_loopback.py and
tests/test_gpu_dia_mask.py.  No mask form exists above 8 diagonals, so none for ND 9.

What no bit test can see: the order in which the diagonals are visited at nd = 1 and nd = 2 (a sum of two terms commutes);
from three terms on a wrong order moves about a third of the rows by an ulp.  The skip-empty-slot select is held by
test_clamped_values (and, at RPT 1 and 2, by the children): with finite operands ``s + 0 * x`` is ``s``."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.support import dia_cases as dc
from tests.support.cheb_ref import cheb_apply_ref, cheb_coefficients
from tests.support.kernel_expect import drain, expect_kernel
from tests.support.poison import bits_equal, poison

pytestmark = pytest.mark.gpu

LD = np.longdouble
gamma = dc.gamma
_MODE = os.environ.get("KRYPY_AMD_SPMV_DIA", "")
_DIA_ON = _MODE != "0"
RPT = {"1": 1, "2": 2}.get(_MODE, 4)                     # row pairs per lane of this process (build_dia)
FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
NAN = np.nan

SQUARE_REAL = tuple(k for k in dc.REAL if k != "rectangular")


def _sum_bar(terms, n=None):
    terms = np.asarray(terms, dtype=LD)
    return gamma(terms.size if n is None else n) * np.abs(terms).sum()


def _poisoned(ctx, n, k=1, dtype=np.float64):
    """A block that holds NaN in every row of every column (its padding stays zero)."""
    return poison(ctx.alloc(n, k, dtype=dtype, zero=False))


def _dtype(c):
    return np.complex128 if c.cplx else np.float64


def _norm_check(nrm, r, what):
    """``nrm`` is the norm of the vector ``r`` the device stored: on the square, gamma_(n+2) (module docstring)."""
    sq = r.astype(LD) ** 2
    assert abs(LD(nrm) ** 2 - sq.sum()) <= _sum_bar(sq, sq.size + 2), "%s: norm %r against %r" % (what, nrm, np.sqrt(sq.sum()))


# ---- the checks (shared with the child processes of test_row_pairs_per_lane) ------------------------------------------------
def check_plan_and_apply(ctx, c, seed=1):
    """(a) + (b): the upload takes what dia_plan says, ONE column through kh_apply has SciPy's bits on every row, the mask
    counter / the complex kernel's counter move as the plan says."""
    plan = c.plan(RPT)
    Ad = ctx.csr(c.A)
    if c.cplx:
        assert Ad.diagonals == 0                      # (the API reports the real banded copies only)
    elif _DIA_ON:
        assert Ad.diagonals == (plan["nd"] if plan["banded"] else 0), "%r: %d diagonals, plan %r" % (c, Ad.diagonals, plan)
    x = dc.vector(c.A.shape[1], 1, seed, cplx=c.cplx)
    X, Y = ctx.upload(x), _poisoned(ctx, c.n, 1, _dtype(c))
    m0, z0 = ctx.get("n_dia_mask"), ctx.get("n_zspmv_dia")
    ctx.apply(Ad, X, 0, Y, 0, 1)
    dm, dz = ctx.get("n_dia_mask") - m0, ctx.get("n_zspmv_dia") - z0
    bits_equal(Y.download()[:, 0], np.asarray(c.A.dot(x[:, 0])), "%r RPT %d: A x" % (c, RPT))
    assert not Y.padding_nonzero(), "%r: padding written" % c
    if _DIA_ON and ctx.get("spmv_dia"):
        assert dm == (1 if plan["masked"] else 0), "%r: n_dia_mask moved by %d, plan %r" % (c, dm, plan)
        if c.cplx and ctx.get("chain_spmv"):
            assert dz == (1 if plan["banded"] else 0), "%r: n_zspmv_dia moved by %d, plan %r" % (c, dz, plan)
    return Ad, X, x


def check_residual(ctx, c, Ad=None, seed=2):
    """(c): R has the bits of b - A.dot(x), the norm is the norm of that R."""
    plan = c.plan(RPT)
    Ad = ctx.csr(c.A) if Ad is None else Ad
    x, b = dc.vector(c.A.shape[1], 1, seed), dc.vector(c.n, 1, seed + 1)
    X, B, R = ctx.upload(x), ctx.upload(b), _poisoned(ctx, c.n)
    m0 = ctx.get("n_dia_mask")
    nrm = ctx.residual(Ad, B, 0, X, 0, R, 0)
    dm = ctx.get("n_dia_mask") - m0
    got = R.download()[:, 0]
    bits_equal(got, b[:, 0] - c.A.dot(x[:, 0]), "%r RPT %d: b - A x" % (c, RPT))
    _norm_check(nrm, got, "%r RPT %d" % (c, RPT))
    assert not R.padding_nonzero(), "%r: padding written" % c
    if _DIA_ON and ctx.get("spmv_dia"):
        assert dm == (1 if plan["masked"] else 0), "%r: n_dia_mask moved by %d" % (c, dm)


def check_cheb(ctx, c, Ad=None, seed=3):
    """(e): kh_cheb_apply of degree 3 (two fused steps), plain and scaled, against tests/support/cheb_ref.py bit for bit."""
    plan = c.plan(RPT)
    Ad = ctx.csr(c.A) if Ad is None else Ad
    A, n, m = c.A, c.n, 3
    lmax = float(np.asarray(abs(A).sum(axis=1)).max())
    coef = cheb_coefficients(lmax / 30.0, lmax, m)
    b = dc.vector(n, 1, seed)
    scale = 1.0 / np.abs(dc.vector(n, 1, seed + 1)[:, 0])
    for dinv in (None, scale):
        Dd = None if dinv is None else ctx.diag(dinv)
        X, Y, S = ctx.upload(b), _poisoned(ctx, n), _poisoned(ctx, n, 3)
        f0, m0 = ctx.get("n_cheb_fused"), ctx.get("n_dia_mask")
        ctx.cheb_apply(Ad, Dd, coef, X, 0, Y, 0, 1, S)
        fused, dm = ctx.get("n_cheb_fused") - f0, ctx.get("n_dia_mask") - m0
        what = "%r RPT %d scaled=%s" % (c, RPT, dinv is not None)
        bits_equal(Y.download(), cheb_apply_ref(A, b, coef, dinv), what)
        assert not Y.padding_nonzero() and not S.padding_nonzero(), "%s: padding written" % what
        on = bool(ctx.get("cheb_fused")) and not FORCED
        expect_kernel(fused == (m - 1 if on else 0), "%s: %d fused launches" % (what, fused))
        if _DIA_ON and ctx.get("spmv_dia"):
            expect_kernel(dm == (m - 1 if plan["masked"] else 0), "%s: n_dia_mask moved by %d" % (what, dm))


def run_catalogue(ctx):
    """What a child process of test_row_pairs_per_lane runs: (a) + (b), (c) and (e) over the whole real catalogue, (f) on its
    six structures."""
    count = 0
    for name in dc.REAL:
        c = dc.case(name)
        assert c.holds(c.plan(RPT)), "%s at RPT %d: %s" % (name, RPT, c.claim)
        Ad, _, _ = check_plan_and_apply(ctx, c)
        check_residual(ctx, c, Ad)
        if name in SQUARE_REAL:
            check_cheb(ctx, c, Ad)
        if name in CLAMP_CASES:
            check_clamped(ctx, c)
        count += 1
    failed = drain()
    assert not failed, "kernel-path expectations: " + "; ".join(failed)
    return count


# ---- a. + b. the plan, EPI_NONE -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.ALL)
def test_apply_one_column(hip, name):
    """detect_dia / build_dia / k_dia_fill / k_dia_mask_fill, then k_spmv_dia<EPI_NONE> (complex: k_zdia_fill, k_zspmv_dia)."""
    c = dc.case(name)
    assert c.holds(), c.claim
    check_plan_and_apply(hip, c)


@pytest.mark.parametrize("name", dc.ALL)
def test_upload_takes_what_the_plan_says(hip, name):
    """``diagonals`` of every real structure; the mask counter moves by exactly one per launch iff the plan says masked."""
    if not _DIA_ON:
        pytest.skip("KRYPY_AMD_SPMV_DIA=0: no banded form")
    c = dc.case(name)
    plan = c.plan(RPT)
    Ad = hip.csr(c.A)
    assert Ad.diagonals == (plan["nd"] if plan["banded"] and not c.cplx else 0), "%r: plan %r" % (c, plan)
    x = dc.vector(c.A.shape[1], 1, 11, cplx=c.cplx)
    X, Y = hip.upload(x), _poisoned(hip, c.n, 1, _dtype(c))
    for rep in range(3):
        m0 = hip.get("n_dia_mask")
        hip.apply(Ad, X, 0, Y, 0, 1)
        assert hip.get("n_dia_mask") - m0 == (1 if plan["masked"] and hip.get("spmv_dia") else 0), (name, rep)


# ---- c. EPI_RES ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.REAL)
def test_residual(hip, name):
    check_residual(hip, dc.case(name))


# ---- d. EPI_DOT ---------------------------------------------------------------------------------------------------------------
DOT_CASES = (["nd%d_value" % k for k in (3, 5, 7, 9, 4)] + ["nd%d_const" % k for k in (3, 5, 7, 4)] +
             ["edge%d_%s" % (n, f) for n in (2047, 2048, 2049, 16385) for f in ("value", "const")])


@pytest.fixture
def per_column(hip):
    """The per-column Gram-Schmidt path of kh_arnoldi_step: chain kernels and the one-reduction form off, put back afterwards."""
    keep = {k: hip.get(k) for k in ("chain", "mgs_lowsync")}
    hip.set("chain", 0)
    hip.set("mgs_lowsync", 0)
    try:
        yield hip
    finally:
        for k, v in keep.items():
            hip.set(k, v)


@pytest.mark.parametrize("name", DOT_CASES)
def test_arnoldi_first_coefficient(per_column, name):
    """EPI_DOT in kh_arnoldi_step (k = 1, start = 0): w = A v_1 with <v_0, w> from the SpMV's epilogue.  The step goes on with
    w -= h_0 v_0, h_1 = <v_1, w>, w -= h_1 v_1, h_2 = ||w||, v_2 = w / h_2 - product and difference rounded separately, so
    NumPy reproduces w and v_2 from the returned coefficients bit for bit."""
    ctx, c = per_column, dc.case(name)
    n = c.n
    Ad = ctx.csr(c.A)
    # entries scaled by a power of two to about 1 / sqrt(n): h_0 v_0 and h_1 v_1 are then some 1 / sqrt(n) of w itself, and a
    # row of A v_1 that is one ulp off still is after the two links (with entries of size 1 the links are a thousand times w
    # and swallow it: the descending-order mutant of the generic loop then moved 2 of 4099 words)
    v = dc.vector(n, 2, 21) * 2.0 ** -int(np.ceil(np.log2(n) / 2))
    V = _poisoned(ctx, n, 3)
    V.upload(0, v)
    W = _poisoned(ctx, n, 2)
    m0 = ctx.get("n_dia_mask")
    h = ctx.arnoldi_step(Ad, None, V, None, W, 0, 1, 0, 1, 0)
    dm = ctx.get("n_dia_mask") - m0
    w = c.A.dot(v[:, 1])
    t0 = v[:, 0].astype(LD) * w.astype(LD)
    assert abs(LD(h[0]) - t0.sum()) <= _sum_bar(t0), "%r: <v0, A v1> = %r against %r" % (c, h[0], t0.sum())
    w1 = w - h[0] * v[:, 0]
    t1 = v[:, 1].astype(LD) * w1.astype(LD)
    assert abs(LD(h[1]) - t1.sum()) <= _sum_bar(t1), "%r: <v1, w> = %r against %r" % (c, h[1], t1.sum())
    w2 = w1 - h[1] * v[:, 1]
    bits_equal(W.download()[:, 0], w2, "%r: w after both links" % c)
    _norm_check(h[2], w2, "%r" % c)
    bits_equal(V.download()[:, 2], w2 / h[2], "%r: v_2" % c)
    assert not V.padding_nonzero() and not W.padding_nonzero()
    if _DIA_ON:
        expect_kernel(dm == (1 if c.plan(RPT)["masked"] else 0), "%r: n_dia_mask moved by %d" % (c, dm))


@pytest.mark.parametrize("name", DOT_CASES)
def test_cg_step(hip, name):
    """EPI_DOT in kh_cg_step(first = 1): Ap with SciPy's bits, <p, Ap> within its bar."""
    ctx, c = hip, dc.case(name)
    n = c.n
    Ad = ctx.csr(c.A)
    p, y, r = dc.vector(n, 1, 31), dc.vector(n, 1, 32), dc.vector(n, 1, 33)
    Pd, APd, Yd, Rd = ctx.upload(p), _poisoned(ctx, n), ctx.upload(y), ctx.upload(r)
    rho = 1.75
    den, rho_new, pap, flags = ctx.cg_step(Ad, None, Pd, 0, APd, 0, Yd, 0, Rd, 0, None, 0, True, 0.0, rho)
    ap = APd.download()[:, 0]
    bits_equal(ap, c.A.dot(p[:, 0]), "%r: Ap" % c)
    terms = p[:, 0].astype(LD) * ap.astype(LD)
    assert abs(LD(den) - terms.sum()) <= _sum_bar(terms), "%r: <p, Ap> = %r against %r" % (c, den, terms.sum())
    assert den == pap
    alpha = rho / den
    bits_equal(Pd.download()[:, 0], p[:, 0], "first = 1 leaves p alone")
    bits_equal(Yd.download()[:, 0], y[:, 0] + alpha * p[:, 0], "%r: yk" % c)
    bits_equal(Rd.download()[:, 0], r[:, 0] - alpha * ap, "%r: r" % c)
    assert not APd.padding_nonzero()


# ---- e. EPI_CHEB --------------------------------------------------------------------------------------------------------------
CHEB_CASES = ["nd%d_%s" % (k, f) for k in (1, 4, 7, 9, 16) for f in ("value", "const")] + ["edge2049_value", "edge2049_const"]


@pytest.mark.parametrize("name", CHEB_CASES)
def test_cheb_epilogue(hip, name):
    check_cheb(hip, dc.case(name))


# ---- f. clamped values --------------------------------------------------------------------------------------------------------
def _same_with_nan(got, want, rows, what):
    """Equal where finite, NaN where NaN (part by part for complex data), and not finite exactly in ``rows``."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert np.array_equal(np.flatnonzero(~np.isfinite(got)), rows), \
        "%s: rows that are not finite %r, predicted %r" % (what, np.flatnonzero(~np.isfinite(got))[:12], rows[:12])
    w = np.float64
    assert np.array_equal(got.view(w), want.view(w), equal_nan=True), "%s: differs from SciPy" % what


CLAMP_CASES = ("far7_value", "far7_const", "nd4_value", "nd4_const", "all_odd_value", "all_odd_const")


def check_clamped(ctx, c):
    """(f): one column, three columns, the residual - with an infinity wherever a clamped load lands."""
    n = c.n
    Ad = ctx.csr(c.A)
    xs, rows = zip(*(dc.edge_vector(c.A, seed) for seed in (7, 8, 9)))
    assert all(np.array_equal(r, rows[0]) for r in rows) and 0 < rows[0].size < 16
    x = np.asfortranarray(np.column_stack(xs))
    b = dc.vector(n, 1, 10)
    with np.errstate(invalid="ignore", over="ignore"):
        want = c.A.dot(x)
        want_r = b[:, 0] - want[:, 1]
    X = ctx.upload(x)
    Y = _poisoned(ctx, n)
    ctx.apply(Ad, X, 0, Y, 0, 1)
    _same_with_nan(Y.download()[:, 0], want[:, 0], rows[0], "%r RPT %d one column" % (c, RPT))
    Y3 = _poisoned(ctx, n, 3)
    s0 = ctx.get("n_spmm")
    ctx.apply(Ad, X, 0, Y3, 0, 3)
    got = Y3.download()
    for j in range(3):
        _same_with_nan(got[:, j], want[:, j], rows[0], "%r three columns, column %d" % (c, j))
    expect_kernel(ctx.get("n_spmm") - s0 == 1, "%r: n_spmm moved by %d" % (c, ctx.get("n_spmm") - s0))
    R = _poisoned(ctx, n)
    ctx.residual(Ad, ctx.upload(b), 0, X, 1, R, 0)
    _same_with_nan(R.download()[:, 0], want_r, rows[0], "%r RPT %d residual" % (c, RPT))
    assert not Y.padding_nonzero() and not Y3.padding_nonzero() and not R.padding_nonzero()


@pytest.mark.parametrize("name", CLAMP_CASES)
def test_clamped_values(hip, name):
    """x[0] = +inf and x[n-1] = -inf: the column of an empty slot is clamped to 0 or n - 1, and only the skip-empty-slot select
    keeps what is loaded there out of the row sum (0 * inf is NaN).  One column, three columns, the residual."""
    check_clamped(hip, dc.case(name))


@pytest.mark.parametrize("name", ["zfar7_4099", "zfar7_513", "z5_4099", "z7_513", "z4"])
def test_clamped_values_complex(hip, name):
    """The same through k_zspmv_dia<5 | 7>: the infinities in the real part of x[0] and x[n-1]."""
    ctx, c = hip, dc.case(name)
    Ad = ctx.csr(c.A)
    x, rows = dc.edge_vector(c.A)
    with np.errstate(invalid="ignore", over="ignore"):
        want = c.A.dot(x)
    X, Y = ctx.upload(x.reshape(-1, 1)), _poisoned(ctx, c.n, 1, np.complex128)
    z0 = ctx.get("n_zspmv_dia")
    ctx.apply(Ad, X, 0, Y, 0, 1)
    dz = ctx.get("n_zspmv_dia") - z0
    got = Y.download()[:, 0]
    assert np.array_equal(np.flatnonzero(~np.isfinite(got)), rows), "%r: rows that are not finite" % c
    assert np.array_equal(got.view(np.float64), want.view(np.float64), equal_nan=True), "%r: differs from SciPy" % c
    assert not Y.padding_nonzero()
    if _DIA_ON and ctx.get("spmv_dia") and ctx.get("chain_spmv"):
        expect_kernel(dz == 1, "%r: n_zspmv_dia moved by %d" % (c, dz))


# ---- g. SpMM ------------------------------------------------------------------------------------------------------------------
def _spmm_operator(kind, n):
    if kind == "nd5_mask":
        A, want = dc.band(n, dc.ND_OFFSETS[5], 805, const=True), (5, True)
    elif kind == "nd8_value":
        A, want = dc.band(n, dc.ND_OFFSETS[8], 808), (8, False)
    elif kind == "nd32":
        A, want = dc.band(n, dc.ND_OFFSETS[32], 832), (32, False)
    elif kind == "far7_value":
        A, want = dc.band(n, dc.FAR7(n), 807), (7, False)
    else:
        A, want = dc.band(n, dc.FAR7(n), 817, const=True), (7, True)
    plan = dc.dia_plan(A)
    assert plan["banded"] and (plan["nd"], plan["masked"]) == want, (kind, n, plan)
    return A, plan


@pytest.mark.parametrize("n", [513, 4099])
@pytest.mark.parametrize("kind", ["nd5_mask", "nd8_value", "nd32", "far7_value", "far7_mask"])
def test_spmm(hip, kind, n):
    """k_spmm_dia<8>: a partial chunk, the chunk tail nc < 8, one full chunk, a second chunk with 1, 8 and 9 columns; the input
    starts at column 1 of X, the output at column 2 of Y, and the two guard columns on either side keep their poison."""
    ctx = hip
    A, plan = _spmm_operator(kind, n)
    Ad = ctx.csr(A)
    if _DIA_ON:
        assert Ad.diagonals == plan["nd"]
    for nc in (2, 7, 8, 9, 16, 17):
        x = dc.vector(n, nc, seed=100 * nc + 1)
        X = ctx.alloc(n, nc + 2)
        X.upload(1, x)
        Y = _poisoned(ctx, n, nc + 4)
        s0, m0 = ctx.get("n_spmm"), ctx.get("n_dia_mask")
        ctx.apply(Ad, X, 1, Y, 2, nc)
        ds, dm = ctx.get("n_spmm") - s0, ctx.get("n_dia_mask") - m0
        got = Y.download()
        guard = np.full((n, 2), NAN)
        bits_equal(got[:, :2], guard, "%s n=%d nc=%d: the columns in front of the output" % (kind, n, nc))
        bits_equal(got[:, 2 + nc:], guard, "%s n=%d nc=%d: the columns behind the output" % (kind, n, nc))
        bits_equal(got[:, 2:2 + nc], A.dot(x), "%s n=%d nc=%d" % (kind, n, nc))
        Y1 = _poisoned(ctx, n, 1)
        for j in range(nc):                               # ... and every column the one-column product's
            ctx.apply(Ad, X, 1 + j, Y1, 0, 1)
            bits_equal(got[:, 2 + j], Y1.download()[:, 0], "%s n=%d nc=%d: column %d against k_spmv_dia" % (kind, n, nc, j))
        assert not Y.padding_nonzero() and not Y1.padding_nonzero()
        expect_kernel(ds == 1, "%s nc=%d: n_spmm moved by %d" % (kind, nc, ds))
        if _DIA_ON and ctx.get("spmv_dia"):
            expect_kernel(dm == ((nc + 7) // 8 if plan["masked"] else 0), "%s nc=%d: n_dia_mask moved by %d" % (kind, nc, dm))


# ---- h. row pairs per lane ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["1", "2"])
def test_row_pairs_per_lane(hip, mode):
    """KRYPY_AMD_SPMV_DIA is read once per process: k_spmv_dia<EPI_NONE | EPI_RES | EPI_CHEB, *, RPT = 1 | 2> run in a child
    process each, over the whole real catalogue with the plan of that mode."""
    code = ("from krypy_amd import _hip\n"
            "from tests import test_gpu_dia as t\n"
            "assert t.RPT == %d\n"
            "print('ok %%d structures at RPT %%d' %% (t.run_catalogue(_hip.get_context()), t.RPT))\n" % int(mode))
    env = dict(os.environ, KRYPY_AMD_SPMV_DIA=mode)
    env.pop("KRYPY_AMD_TEST_FORCE_MULTI", None)
    env.pop("KRYPY_AMD_FORCE_MULTI", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and ("ok %d structures at RPT %s" % (len(dc.REAL), mode)) in out.stdout, \
        (out.stdout[-500:], out.stderr[-2000:])


# ---- i. split launches --------------------------------------------------------------------------------------------------------
@pytest.fixture
def loop_ctx(hip):
    """A 1-rank communicator in forced multi-rank mode (tests/test_gpu_halo_loopback.py): an operator without ghost columns
    gets a one-block boundary at both ends, so an SpMV is an interior launch and a boundary launch."""
    from krypy_amd import _hip

    os.environ["KRYPY_AMD_FORCE_MULTI"] = "1"
    try:
        ctx = _hip.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
    finally:
        del os.environ["KRYPY_AMD_FORCE_MULTI"]
    yield ctx
    ctx.close()


@pytest.mark.parametrize("form", ["value", "const"])
@pytest.mark.parametrize("n", [2048, 4096, 4097, 16385])
def test_split_launches(loop_ctx, n, form):
    """1, 2, 3 and 9 workgroups at 4 row pairs per lane: no split with 1 or 2 blocks, one interior and two boundary blocks
    with 3, seven and two with 9.  The vectors of the product and of the residual have the unsplit run's bits (and SciPy's),
    the norm - partial sums from two launches - stays within its bar."""
    ctx, c = loop_ctx, dc.case("edge%d_%s" % (n, form))
    plan = c.plan(RPT)
    Ad = ctx.csr(c.A)
    ctx.set_halo(Ad, 0, 0, 0, 0)
    nblk = plan["nblk"]
    lo, hi = min(1, nblk), max(nblk - 1, min(1, nblk))
    split = 1 if (lo < hi and (lo > 0 or hi < nblk)) else 0
    if RPT == 4:
        assert (nblk, split) == {2048: (1, 0), 4096: (2, 0), 4097: (3, 1), 16385: (9, 1)}[n]
    x, b = dc.vector(n, 1, 41), dc.vector(n, 1, 42)
    X, B = ctx.upload(x), ctx.upload(b)
    out = {}
    for on in (1, 0):
        ctx.set("spmv_split", on)
        Y, R = _poisoned(ctx, n), _poisoned(ctx, n)
        s0 = ctx.get("n_spmv_split")
        ctx.apply(Ad, X, 0, Y, 0, 1)
        s1 = ctx.get("n_spmv_split")
        nrm = ctx.residual(Ad, B, 0, X, 0, R, 0)
        s2 = ctx.get("n_spmv_split")
        out[on] = (Y.download()[:, 0], R.download()[:, 0], nrm)
        assert not Y.padding_nonzero() and not R.padding_nonzero()
        if _DIA_ON:
            expect_kernel((s1 - s0, s2 - s1) == (split * on, split * on),
                          "n=%d %s split=%d: n_spmv_split moved by %r" % (n, form, on, (s1 - s0, s2 - s1)))
    ctx.set("spmv_split", 1)
    bits_equal(out[1][0], out[0][0], "n=%d %s: product, split against unsplit" % (n, form))
    bits_equal(out[1][1], out[0][1], "n=%d %s: residual, split against unsplit" % (n, form))
    bits_equal(out[1][0], c.A.dot(x[:, 0]), "n=%d %s: product" % (n, form))
    bits_equal(out[1][1], b[:, 0] - c.A.dot(x[:, 0]), "n=%d %s: residual" % (n, form))
    for on in (1, 0):
        _norm_check(out[on][2], out[on][1], "n=%d %s split=%d" % (n, form, on))
