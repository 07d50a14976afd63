"""GPU tests of the CSR-stream SpMV / SpMM (k_spmv_stream, k_spmm_stream, k_zspmv_stream) at every tile kh_ctx_tune accepts,
at the edges of the LDS window's decision rule and of the row-block geometry, and of every reduction / streaming kernel whose
grid kh_ctx_tune's reduce_blocks bounds.  The structures and the replica of the host-side plan: tests/support/csr_stream_cases.py
(held on the CPU by tests/test_csr_stream_host.py).

Bars.  Bit equality is against SciPy / NumPy, the library's contract, on every row except the rows longer than the tile, which
the structure names.  Every floating-point bar is the bound of a sum of m terms in ANY order, gamma_m * sum |terms| with
gamma_m = m u / (1 - m u), u = 2^-53, against a ``longdouble`` reference.  Operand magnitudes lie in [1, 2): a lost or repeated
term moves a sum by at least 1, the bound stays below 1e-3 at every size used."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import csr_stream_cases as cs
from tests.support.cheb_ref import cheb_apply_ref, cheb_coefficients
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = cs.U
gamma = cs.gamma


# ---- the context, tuned ---------------------------------------------------------------------------------------------------
@pytest.fixture
def tuned(hip):
    """``tuned(tile=T, reduce_blocks=B)`` tunes the context (before any operator is uploaded: the tile is read at upload) and
    returns it; tile 2048, the reduction grid and the switches the tests move are put back afterwards."""
    nb0 = hip.info()["reduce_blocks"]
    before = {k: hip.get(k) for k in ("spmv_win", "spmv_dia")}

    def tune(tile=0, reduce_blocks=0):
        hip.tune(reduce_blocks=reduce_blocks, spmv_tile=tile)
        return hip

    tune.default_reduce_blocks = nb0
    try:
        yield tune
    finally:
        hip.tune(reduce_blocks=nb0, spmv_tile=2048)
        for k, v in before.items():
            hip.set(k, v)


def _upload(ctx, c, win=1):
    """The operator of a catalogue case under the switches it asks for."""
    ctx.set("spmv_win", win)
    for k, v in c.switches.items():
        ctx.set(k, v)
    Ad = ctx.csr(c.A)
    assert Ad.diagonals == 0 or c.switches.get("spmv_dia") == 0, "%r got a banded form" % c
    return Ad


def _tile_in_use(ctx):
    """The tile an upload takes now, seen from outside: ONE row of L entries within L columns goes through the LDS window
    exactly when L <= tile (a longer row is no block that fits)."""
    keep = ctx.get("spmv_win")
    ctx.set("spmv_win", 1)
    tile = 0
    try:
        for L in cs.TILES:
            A = sp.csr_matrix((np.ones(L), np.arange(L), [0, L]), shape=(1, L))
            Ad, X, Y = ctx.csr(A), ctx.upload(np.ones(L)), ctx.alloc(1, 1)
            w0 = ctx.get("n_spmv_win")
            ctx.apply(Ad, X, 0, Y, 0, 1)
            assert Y.download()[0, 0] == float(L)
            if ctx.get("n_spmv_win") - w0 == 1:
                tile = L
    finally:
        ctx.set("spmv_win", keep)
    return tile


# ---- references -----------------------------------------------------------------------------------------------------------
def _row_terms(A, x, r):
    """The products of row ``r`` as longdouble arrays: (terms of the real part, terms of the imaginary part or None)."""
    z0, z1 = A.indptr[r], A.indptr[r + 1]
    a, v = A.data[z0:z1], x[A.indices[z0:z1]]
    if np.iscomplexobj(a) or np.iscomplexobj(v):
        ar, ai, vr, vi = (np.asarray(t, dtype=LD) for t in (np.real(a), np.imag(a), np.real(v), np.imag(v)))
        return np.concatenate([ar * vr, -(ai * vi)]), np.concatenate([ar * vi, ai * vr])
    return np.asarray(a, dtype=LD) * np.asarray(v, dtype=LD), None


def _check_product(c, X, got, what, tile=None):
    """``got == A.dot(X)`` bit for bit on every row that fits the tile; a longer row within
    ``gamma_cnt * sum_j |a_ij x_j|`` of the longdouble sum (any summation order; complex: on the modulus)."""
    A = c.A
    tile = c.tile if tile is None else tile
    long_rows = np.nonzero(np.diff(A.indptr) > tile)[0]
    assert np.array_equal(long_rows, c.long_rows) or tile != c.tile
    want = np.asarray(A.dot(X)).reshape(got.shape)
    keep = np.ones(A.shape[0], dtype=bool)
    keep[long_rows] = False
    bad = np.nonzero((got[keep] != want[keep]).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ from SciPy, first at kept row %d" % (what, bad.size, bad[0])
    for r in long_rows:
        cnt = int(A.indptr[r + 1] - A.indptr[r])
        for j in range(X.shape[1]):
            re, im = _row_terms(A, X[:, j], r)
            if im is None:
                err, bar = abs(LD(got[r, j]) - re.sum()), gamma(cnt) * np.abs(re).sum()
            else:
                a, v = np.abs(A.data[A.indptr[r]:A.indptr[r + 1]]).astype(LD), np.abs(X[A.indices[A.indptr[r]:A.indptr[r + 1]], j])
                err = np.hypot(LD(got[r, j].real) - re.sum(), LD(got[r, j].imag) - im.sum())
                bar = gamma(cnt) * (a * v.astype(LD)).sum()
            assert err <= bar, "%s: long row %d column %d off by %.3e, bar %.3e" % (what, r, j, err, bar)


def _sum_bar(terms, n=None):
    terms = np.asarray(terms, dtype=LD)
    return gamma(terms.size if n is None else n) * np.abs(terms).sum()


# ---- a. SpMV bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win", [1, 0])
@pytest.mark.parametrize("T", cs.TILES)
@pytest.mark.parametrize("name", sorted(cs.REAL))
def test_spmv_bits(tuned, name, T, win):
    """k_spmv_stream<EPI_NONE, T / 256, WIN>: every structure, every tile, with the window allowed and switched off."""
    c = cs.case(name, T)
    assert c.holds(), c.claim
    ctx = tuned(tile=T)
    Ad = _upload(ctx, c, win)
    x = cs.vector(c.A.shape[1], 1, seed=T + win)
    X, Y = ctx.upload(x), ctx.alloc(c.A.shape[0], 1)
    w0 = ctx.get("n_spmv_win")
    ctx.apply(Ad, X, 0, Y, 0, 1)
    used = ctx.get("n_spmv_win") - w0
    _check_product(c, x, Y.download(), "%r win=%d" % (c, win))
    assert used == (1 if c.plan["window_on"] and win else 0), "%r win=%d: n_spmv_win moved by %d" % (c, win, used)


def test_tile_is_read_at_upload(tuned):
    """The probe behind test (f), and the fixture's contract: after tune(T) an upload takes tile T."""
    for T in cs.TILES:
        assert _tile_in_use(tuned(tile=T)) == T


# ---- b. epilogues ----------------------------------------------------------------------------------------------------------
EPI_CASES = ("all_fit", "nine_of_ten", "full_row_win", "full_row_nowin", "many_short_rows")


@pytest.mark.parametrize("T", cs.TILES)
@pytest.mark.parametrize("name", EPI_CASES)
def test_residual_epilogue(tuned, name, T):
    """EPI_RES: R has the bits of b - A.dot(x), the norm is the norm of that R."""
    c = cs.case(name, T)
    ctx = tuned(tile=T)
    Ad = _upload(ctx, c)
    n = c.A.shape[0]
    x, b = cs.vector(n, 1, seed=3 * T), cs.vector(n, 1, seed=3 * T + 1)
    X, B, R = ctx.upload(x), ctx.upload(b), ctx.alloc(n, 1)
    w0 = ctx.get("n_spmv_win")
    nrm = ctx.residual(Ad, B, 0, X, 0, R, 0)
    used = ctx.get("n_spmv_win") - w0
    got = R.download()
    # b - (A x): the row sum is the product's, the subtraction one more rounding - the long rows against b - (their device sum)
    keep = np.ones(n, dtype=bool)
    keep[c.long_rows] = False
    want = b[:, 0] - c.A.dot(x[:, 0])
    assert np.array_equal(got[keep, 0], want[keep]), "%r: R differs from b - A.dot(x)" % c
    for r in c.long_rows:
        re, _ = _row_terms(c.A, x[:, 0], r)
        cnt = re.size
        err = abs(LD(got[r, 0]) - (LD(b[r, 0]) - re.sum()))
        bar = gamma(cnt + 1) * (np.abs(re).sum() + abs(b[r, 0]))
        assert err <= bar, "%r: long row %d of R off by %.3e, bar %.3e" % (c, r, err, bar)
    ref = np.sqrt((got[:, 0].astype(LD) ** 2).sum())
    assert abs(LD(nrm) - ref) <= (gamma(n) / 2 + U) * ref, "%r: norm %r against %r" % (c, nrm, ref)
    assert used == (1 if c.plan["window_on"] else 0), "%r: n_spmv_win moved by %d" % (c, used)


def _positive_direction(A, seed):
    """A direction p with magnitudes in [1, 2) and <p, A p> safely positive (these operators are indefinite: the first of a
    seeded sequence whose extended-precision <p, A p> is positive with room to spare)."""
    n = A.shape[0]
    for s in range(seed, seed + 200):
        p = cs.vector(n, 1, seed=s)
        terms = p[:, 0].astype(LD) * np.asarray(A.dot(p[:, 0]), dtype=LD)
        if terms.sum() > 1e-3 * np.abs(terms).sum():
            return p
    raise AssertionError("no direction with <p, A p> > 0 among 200 seeds")


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("T", cs.TILES)
@pytest.mark.parametrize("name", EPI_CASES)
def test_cg_step_epilogue(tuned, name, T, jacobi):
    """EPI_DOT inside kh_cg_step(first = 1): Ap, <p, Ap>, the step taken with rho / <p, Ap>, the sanity word."""
    c = cs.case(name, T)
    ctx = tuned(tile=T)
    Ad = _upload(ctx, c)
    A, n = c.A, c.A.shape[0]
    p = _positive_direction(A, 5 * T)
    r, y = cs.vector(n, 1, seed=5 * T + 1), cs.vector(n, 1, seed=5 * T + 2)
    d = np.abs(cs.vector(n, 1, seed=5 * T + 3)[:, 0])
    Pd, APd, Yd, Rd = ctx.upload(p), ctx.alloc(n, 1), ctx.upload(y), ctx.upload(r)
    Md = ctx.diag(d) if jacobi else None
    Zd = ctx.alloc(n, 1) if jacobi else None
    rho = 1.75
    w0 = ctx.get("n_spmv_win")
    den, rho_new, pap, flags = ctx.cg_step(Ad, Md, Pd, 0, APd, 0, Yd, 0, Rd, 0, Zd, 0, True, 0.0, rho)
    used = ctx.get("n_spmv_win") - w0
    ap = APd.download()
    _check_product(c, p, ap, "%r Ap" % c)
    assert np.array_equal(Pd.download(), p), "first = 1 leaves p alone"
    terms = p[:, 0].astype(LD) * ap[:, 0].astype(LD)
    assert abs(LD(den) - terms.sum()) <= _sum_bar(terms), "%r: <p, Ap> = %r against %r" % (c, den, terms.sum())
    assert den == pap and flags == 0, (den, pap, flags)
    alpha = rho / den                                     # the IEEE division the device made
    rn = r[:, 0] - alpha * ap[:, 0]
    assert np.array_equal(Yd.download()[:, 0], y[:, 0] + alpha * p[:, 0]), "%r: yk" % c
    assert np.array_equal(Rd.download()[:, 0], rn), "%r: r" % c
    zn = rn
    if jacobi:
        zn = d * rn
        assert np.array_equal(Zd.download()[:, 0], zn), "%r: z" % c
    rz = rn.astype(LD) * zn.astype(LD)
    assert abs(LD(rho_new) - rz.sum()) <= _sum_bar(rz), "%r: rho_new = %r against %r" % (c, rho_new, rz.sum())
    assert used == (1 if c.plan["window_on"] else 0), "%r: n_spmv_win moved by %d" % (c, used)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("T", cs.TILES)
@pytest.mark.parametrize("name", ["nine_of_ten", "full_row_win", "full_row_nowin"])
def test_cheb_epilogue(tuned, name, T, scaled):
    """EPI_CHEB: the bits of tests/support/cheb_ref.py.  Degree 2 is ONE fused step, so a row longer than the tile keeps its
    rounding to itself: z_i = d0_i + ((a d0_i) + b ((r_i - s_i) [* dinv_i])) with its own row sum s_i, and the other rows'
    bits are the oracle's.  Degree 3 follows on nine_of_ten, where no row is long."""
    c = cs.case(name, T)
    ctx = tuned(tile=T)
    Ad = _upload(ctx, c)
    A, n = c.A, c.A.shape[0]
    lmax = float(np.asarray(abs(A).sum(axis=1)).max())
    dinv = 1.0 / np.abs(cs.vector(n, 1, seed=7 * T)[:, 0]) if scaled else None
    Dd = ctx.diag(dinv) if scaled else None
    b = cs.vector(n, 1, seed=7 * T + 1)
    keep = np.ones(n, dtype=bool)
    keep[c.long_rows] = False
    for m in ((2,) if c.long_rows.size else (2, 3)):
        coef = cheb_coefficients(lmax / 30.0, lmax, m)
        X, Y, S = ctx.upload(b), ctx.alloc(n, 1, zero=False), ctx.alloc(n, 3, zero=False)
        f0, w0 = ctx.get("n_cheb_fused"), ctx.get("n_spmv_win")
        ctx.cheb_apply(Ad, Dd, coef, X, 0, Y, 0, 1, S)
        fused, used = ctx.get("n_cheb_fused") - f0, ctx.get("n_spmv_win") - w0
        got, want = Y.download()[:, 0], cheb_apply_ref(A, b, coef, dinv)[:, 0]
        assert np.array_equal(got[keep], want[keep]), "%r degree %d scaled=%s: not the oracle's bits" % (c, m, scaled)
        for r in c.long_rows:
            # step 0: d0 = b0 * (r [* dinv]) = z0 (exact to the oracle: row-local); step 1 with the row sum s of A z0
            sc = 1.0 if dinv is None else dinv[r]
            z0 = cheb_apply_ref(A, b, coef[:1], dinv)[:, 0]
            d0 = z0[r]
            re, _ = _row_terms(A, z0, r)
            a1, b1 = LD(coef[1][0]), LD(coef[1][1])
            exact = LD(d0) + (a1 * LD(d0) + b1 * ((LD(b[r, 0]) - re.sum()) * LD(sc)))
            # cnt roundings of the sum and five of the row's own operations, on the magnitudes that enter them
            mags = abs(b1) * abs(LD(sc)) * (abs(LD(b[r, 0])) + np.abs(re).sum()) + abs(a1 * LD(d0)) + abs(LD(d0))
            assert abs(LD(got[r]) - exact) <= gamma(re.size + 5) * mags, "%r degree 2: long row %d" % (c, r)
        expect_kernel(fused in (m - 1, 0), "%r: %d fused launches" % (c, fused))
        if fused == m - 1:
            expect_kernel(used == ((m - 1) if c.plan["window_on"] else 0), "%r: n_spmv_win moved by %d" % (c, used))


# ---- c. SpMM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", cs.TILES)
@pytest.mark.parametrize("name", ["all_fit", "full_row_win", "full_row_nowin", "many_short_rows", "rect_tail"])
def test_spmm_bits(tuned, name, T):
    """k_spmm_stream<T / 256, 4>: one partial chunk of four columns, full chunks with and without a tail; X and Y at column
    offsets, the columns around the output untouched.  T = 4096 is the launch with 128 KB of dynamic LDS."""
    c = cs.case(name, T)
    ctx = tuned(tile=T)
    Ad = _upload(ctx, c)
    nr, ncol = c.A.shape
    for k in (2, 3, 4, 5, 7, 8, 13):
        x = cs.vector(ncol, k, seed=11 * T + k)
        y0 = cs.vector(nr, k + 4, seed=11 * T + 100 + k)
        X = ctx.alloc(ncol, k + 2)
        X.upload(1, x)
        Y = ctx.upload(y0)
        s0 = ctx.get("n_spmm")
        ctx.apply(Ad, X, 1, Y, 2, k)
        assert ctx.get("n_spmm") - s0 == 1, "%r k=%d: n_spmm moved by %d" % (c, k, ctx.get("n_spmm") - s0)
        got = Y.download()
        assert np.array_equal(got[:, :2], y0[:, :2]) and np.array_equal(got[:, 2 + k:], y0[:, 2 + k:]), \
            "%r k=%d: columns beside the output were written" % (c, k)
        _check_product(c, x, got[:, 2:2 + k], "%r k=%d" % (c, k))


# ---- d. complex ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", cs.ZTILES)
@pytest.mark.parametrize("name", sorted(cs.COMPLEX))
def test_complex_spmv_bits(tuned, name, T):
    """k_zspmv_stream<T / 256> with one and with three columns."""
    c = cs.zcase(name, T)
    ctx = tuned(tile=T)
    Ad = ctx.csr(c.A)
    n = c.A.shape[0]
    for k in (1, 3):
        x = cs.vector(n, k, seed=13 * T + k, cplx=True)
        X, Y = ctx.upload(x), ctx.alloc(n, k, dtype=complex)
        ctx.apply(Ad, X, 0, Y, 0, k)
        _check_product(c, x, Y.download(), "complex %r k=%d" % (c, k))


@pytest.mark.parametrize("name", sorted(cs.COMPLEX))
def test_complex_operator_of_a_context_tuned_to_4096_runs_at_2048(tuned, name):
    """kh_zcsr_upload caps the tile at 2048 (k_zspmv_stream<16> cannot be reached): the bits of the 2048 run - the row of 2049
    entries included, which a tile of 4096 would have added left to right."""
    c = cs.zcase(name, 2048)
    n = c.A.shape[0]
    x = cs.vector(n, 3, seed=17, cplx=True)
    out = []
    for T in (2048, 4096):
        ctx = tuned(tile=T)
        Ad = ctx.csr(c.A)
        X, Y = ctx.upload(x), ctx.alloc(n, 3, dtype=complex)
        ctx.apply(Ad, X, 0, Y, 0, 3)
        out.append(Y.download())
    _check_product(c, x, out[1], "complex %r tuned to 4096" % c, tile=2048)
    assert np.array_equal(out[0], out[1]), "%r: the run tuned to 4096 differs from 2048's" % c


# ---- e. the reduction grid -------------------------------------------------------------------------------------------------
def _dot_check(got, V, w, what):
    for j in range(V.shape[1]):
        if np.iscomplexobj(V):
            vr, vi, wr, wi = (np.asarray(t, dtype=LD) for t in (V[:, j].real, V[:, j].imag, w.real, w.imag))
            re, im = np.concatenate([vr * wr, vi * wi]), np.concatenate([vr * wi, -(vi * wr)])      # conj(v) w
            assert abs(LD(got[j].real) - re.sum()) <= _sum_bar(re) and abs(LD(got[j].imag) - im.sum()) <= _sum_bar(im), \
                "%s: column %d: %r against (%r, %r)" % (what, j, got[j], re.sum(), im.sum())
        else:
            terms = V[:, j].astype(LD) * w.astype(LD)
            assert abs(LD(got[j]) - terms.sum()) <= _sum_bar(terms), "%s: column %d: %r against %r" % (what, j, got[j], terms.sum())


def _cg_update_check(ctx, n, seed, jacobi, what):
    p, ap, y, r = (cs.vector(n, 1, seed=seed + i) for i in range(4))
    d = np.abs(cs.vector(n, 1, seed=seed + 4)[:, 0])
    alpha = 0.40625
    rn = r[:, 0] - alpha * ap[:, 0]
    zn = d * rn if jacobi else rn
    rz = rn.astype(LD) * zn.astype(LD)
    Md = ctx.diag(d) if jacobi else None
    rhos = []
    for _ in range(2):
        Pd, APd, Yd, Rd = ctx.upload(p), ctx.upload(ap), ctx.upload(y), ctx.upload(r)
        Zd = ctx.alloc(n, 1) if jacobi else None
        rho = ctx.cg_update(alpha, Pd, 0, APd, 0, Yd, 0, Rd, 0, Md, Zd, 0)
        assert np.array_equal(Yd.download()[:, 0], y[:, 0] + alpha * p[:, 0]), "%s: yk" % what
        assert np.array_equal(Rd.download()[:, 0], rn), "%s: r" % what
        if jacobi:
            assert np.array_equal(Zd.download()[:, 0], zn), "%s: z" % what
        assert abs(LD(rho) - rz.sum()) <= _sum_bar(rz), "%s: <r, z> = %r against %r" % (what, rho, rz.sum())
        rhos.append(rho)
    assert rhos[0] == rhos[1], "%s: <r, z> differs between two runs" % what


def _streaming_check(ctx, n, seed, what):
    """k_waxpby, k_vdiv, k_minres_update, k_cheb_update: no sum - NumPy's bits at every grid."""
    a, b, c3, d4, e5 = (cs.vector(n, 1, seed=seed + i)[:, 0] for i in range(5))
    A_, B_, Z = ctx.upload(a), ctx.upload(b), ctx.alloc(n, 1)
    ctx.waxpby(Z, 0, 1.375, A_, 0, -0.8125, B_, 0)
    assert np.array_equal(Z.download()[:, 0], (1.375 * a) + (-0.8125 * b)), "%s: waxpby" % what
    ctx.vdiv(Z, 0, A_, 0, 1.7)
    assert np.array_equal(Z.download()[:, 0], a / 1.7), "%s: vdiv" % what
    # z = ((v - r0 w0) - r1 w1) / r2 over w0; yk += y0 z
    V, W, Y = ctx.upload(np.column_stack([a, b])), ctx.upload(np.column_stack([c3, d4])), ctx.upload(e5)
    r0, r1, r2, y0 = 0.3125, -1.21, 1.3, 0.77
    ctx.minres_update(V, 1, W, 0, r0, r1, r2, y0, Y, 0)
    z = ((b - r0 * c3) - r1 * d4) / r2
    got = W.download()
    assert np.array_equal(got[:, 0], z) and np.array_equal(got[:, 1], d4), "%s: minres_update" % what
    assert np.array_equal(Y.download()[:, 0], e5 + y0 * z), "%s: minres_update (yk)" % what
    # d = (ca d) + (cb ((r - az) * dinv)); z_out = z_in + d
    dinv = np.abs(e5)
    AZ, R, D, Zin, Zout, Dd = ctx.upload(a), ctx.upload(b), ctx.upload(c3), ctx.upload(d4), ctx.alloc(n, 1), ctx.diag(dinv)
    ca, cb = 0.4375, 1.1
    ctx.cheb_update(AZ, 0, R, 0, Dd, D, 0, Zin, 0, Zout, 0, ca, cb)
    dn = (ca * c3) + (cb * ((b - a) * dinv))
    assert np.array_equal(D.download()[:, 0], dn) and np.array_equal(Zout.download()[:, 0], d4 + dn), "%s: cheb_update" % what


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
@pytest.mark.parametrize("nb", [1, 3, "default", 4096])
def test_reductions_and_streaming_kernels_at_every_grid(tuned, nb, n):
    """k_multidot (16 + 2 + 1 columns), k_zmultidot, the norm, kh_gemm_tn, k_cg_update and the streaming kernels with the
    reduction grid at its smallest, at an odd size, at the default and at the ABI's maximum."""
    ctx = tuned(reduce_blocks=tuned.default_reduce_blocks if nb == "default" else nb)
    assert ctx.info()["reduce_blocks"] == (tuned.default_reduce_blocks if nb == "default" else nb)
    what = "reduce_blocks=%s n=%d" % (nb, n)
    V, w = cs.vector(n, 19, seed=n), cs.vector(n, 1, seed=n + 1)
    Vd, Wd = ctx.upload(V), ctx.upload(w)
    for k in (1, 5, 16, 19):
        got = ctx.dot_panel(Vd, 19 - k, k, Wd, 0)
        _dot_check(got, V[:, 19 - k:], w[:, 0], "%s dot_panel(%d)" % (what, k))
        assert np.array_equal(got, ctx.dot_panel(Vd, 19 - k, k, Wd, 0)), "%s dot_panel(%d): two runs differ" % (what, k)
    ZV, zw = cs.vector(n, 19, seed=n + 2, cplx=True), cs.vector(n, 1, seed=n + 3, cplx=True)
    ZVd, ZWd = ctx.upload(ZV), ctx.upload(zw)
    got = ctx.dot_panel(ZVd, 0, 19, ZWd, 0)
    _dot_check(got, ZV, zw[:, 0], "%s complex dot_panel(19)" % what)
    assert np.array_equal(got, ctx.dot_panel(ZVd, 0, 19, ZWd, 0)), "%s complex dot_panel: two runs differ" % what
    nrm = ctx.nrm2(Wd, 0)
    ref = np.sqrt((w[:, 0].astype(LD) ** 2).sum())
    assert abs(LD(nrm) - ref) <= (gamma(n) / 2 + U) * ref and nrm == ctx.nrm2(Wd, 0), "%s nrm2: %r against %r" % (what, nrm, ref)
    G = ctx.gemm_tn(Vd, 2, 7, Wd, 0, 1)
    _dot_check(G[:, 0], V[:, 2:9], w[:, 0], "%s gemm_tn" % what)
    assert np.array_equal(G, ctx.gemm_tn(Vd, 2, 7, Wd, 0, 1)), "%s gemm_tn: two runs differ" % what
    for jacobi in (False, True):
        _cg_update_check(ctx, n, n + 10, jacobi, "%s cg_update jacobi=%s" % (what, jacobi))
    _streaming_check(ctx, n, n + 20, what)


def test_partials_up_to_the_last_double_of_the_allocation(tuned):
    """reduce_blocks = 4096 and n = 2 * 4096 * 256 + 7: grid_lin returns 8192 and k_cg_update's last partial is the last double
    of ctx->part (slot SLOT_NRM and the spare one behind it: tests/test_csr_stream_host.py holds the arithmetic).  Afterwards
    the neighbouring slots still serve: 16 inner products and a norm on fresh data."""
    ctx = tuned(reduce_blocks=4096)
    n = 2 * 4096 * 256 + 7
    _cg_update_check(ctx, n, 31, True, "cg_update at 8192 workgroups")
    # kh_cg_step on a diagonal operator: k_diag_apply, the inner product through slot 0, k_cg_update reading it
    a = np.abs(cs.vector(n, 1, seed=41)[:, 0])
    p, y, r = (cs.vector(n, 1, seed=42 + i) for i in range(3))
    Ad, Pd, APd, Yd, Rd = ctx.diag(a), ctx.upload(p), ctx.alloc(n, 1), ctx.upload(y), ctx.upload(r)
    rho = 1.75
    den, rho_new, pap, flags = ctx.cg_step(Ad, None, Pd, 0, APd, 0, Yd, 0, Rd, 0, None, 0, True, 0.0, rho)
    ap = a * p[:, 0]
    assert np.array_equal(APd.download()[:, 0], ap)
    terms = p[:, 0].astype(LD) * ap.astype(LD)
    assert abs(LD(den) - terms.sum()) <= _sum_bar(terms) and flags == 0 and den == pap, (den, terms.sum(), flags)
    alpha = rho / den
    rn = r[:, 0] - alpha * ap
    assert np.array_equal(Yd.download()[:, 0], y[:, 0] + alpha * p[:, 0]) and np.array_equal(Rd.download()[:, 0], rn)
    rz = rn.astype(LD) ** 2
    assert abs(LD(rho_new) - rz.sum()) <= _sum_bar(rz), (rho_new, rz.sum())
    m = 100003
    V, w = cs.vector(m, 16, seed=51), cs.vector(m, 1, seed=52)
    Vd, Wd = ctx.upload(V), ctx.upload(w)
    _dot_check(ctx.dot_panel(Vd, 0, 16, Wd, 0), V, w[:, 0], "dot_panel(16) after the widest grid")
    ref = np.sqrt((w[:, 0].astype(LD) ** 2).sum())
    assert abs(LD(ctx.nrm2(Wd, 0)) - ref) <= (gamma(m) / 2 + U) * ref


# ---- f. argument errors ----------------------------------------------------------------------------------------------------
def test_tune_rejects_bad_arguments_and_changes_nothing(tuned):
    from krypy_amd._hip import BackendError

    ctx = tuned(tile=1024, reduce_blocks=77)
    for kw in (dict(spmv_tile=3000), dict(reduce_blocks=4097), dict(reduce_blocks=5, spmv_tile=3000),
               dict(reduce_blocks=4097, spmv_tile=4096)):
        with pytest.raises(BackendError):
            ctx.tune(**kw)
        assert ctx.info()["reduce_blocks"] == 77, "after tune(%r)" % kw
        assert _tile_in_use(ctx) == 1024, "after tune(%r)" % kw
    ctx.tune()                                            # zeros keep what is set
    assert ctx.info()["reduce_blocks"] == 77 and _tile_in_use(ctx) == 1024
