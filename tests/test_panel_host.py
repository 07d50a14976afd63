"""CPU side of tests/test_gpu_panel.py: the catalogue's predicates hold, the restated split plans agree with brute force, the
constants the GPU tests rely on are what the sources say (and the arithmetic the C code assumes about them holds), and the
order-exact references of tests/support/panel_ref.py agree with its extended-precision ones within the textbook bound."""
import os
import re

import numpy as np
import pytest

from tests.support import panel_cases as pc
from tests.support import panel_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = pr.LD


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"constexpr\s+int(?:64_t)?\s+(?:\w+\s*=\s*[\w+ ]+,\s*)*?%s\s*=\s*(\d+)\s*[;,]" % name, text)
    assert m, "constant %s not found" % name
    return int(m.group(1))


# ---- the catalogue -----------------------------------------------------------------------------------------------------------
def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).nmant >= 63, "the extended references need an 80-bit longdouble"


def test_every_case_selects_the_edges_it_claims():
    assert {(c.path, c.width) for c in pc.CASES} == {("real", w) for w in pc.REAL_WIDTHS} | {("c128", w) for w in pc.C128_WIDTHS}
    for c in pc.CASES:
        assert c.edges, "%r selects no edge" % (c,)
        for name in c.edges:
            assert pc.EDGES[name](c.path, c.width), "%r: %s" % (c, name)
        assert c.rows == ((pc.WIDE_ROWS,) if c.width >= pc.WIDE_FROM else pc.ROWS)


def test_every_edge_is_reached_on_the_path_it_exists_on():
    for path, names in pc.REQUIRED.items():
        reached = {n for c in pc.CASES if c.path == path for n in c.edges}
        assert set(names) <= reached, "%s: nobody selects %s" % (path, sorted(set(names) - reached))
    # the named anchors of the catalogue
    by = {(c.path, c.width): c.edges for c in pc.CASES}
    assert pr.split_real(47) == [16, 16, 8, 4, 2, 1] and "every chunk size in one call" in by[("real", 47)]
    assert "second outer chunk of dot_panel_dev: out_dev + done" in by[("real", 17)]
    assert "exactly at the cap: the coefficients fill SC_COEF ... SC_LS" in by[("real", 1024)] and \
        "exactly at the cap: the coefficients fill SC_COEF ... SC_LS" in by[("c128", 512)]
    assert "wrapper splits: a second C call of one column" in by[("real", 1025)] and \
        "wrapper splits: a second C call of one column" in by[("c128", 513)]


def test_pass_edges_of_gemm_nn():
    for ks, per in ((pc.GEMM_K, pr.KMAX), (pc.ZGEMM_K, pr.ZCAP)):
        reached = set()
        for k in ks:
            e = pc.k_edges(k, per)
            assert e, "k = %d selects no edge of passes of %d" % (k, per)
            reached.update(e)
        assert reached == set(pc.K_EDGES), sorted(set(pc.K_EDGES) - reached)
    assert pr.passes(2049, pr.KMAX) == [1024, 1024, 1] and pr.passes(1025, pr.ZCAP) == [512, 512, 1]
    for k in pc.MFMA_K:
        assert len(pr.passes(k, pr.KP)) > 3, "k_panel_gemm_mfma beyond three passes of 64"
    assert [len(pr.passes(k, pr.KP)) for k in pc.MFMA_K] == [16, 17, 18] and pr.passes(1025, pr.KP)[-1] == 1
    assert all(2 <= nc <= 16 for nc in pc.MFMA_NC + pc.GEMM_NC_OFF) and all(nc == 1 or nc > 16 for nc in pc.GEMM_NC)


# ---- the split plans against brute force ---------------------------------------------------------------------------------------
def _fewest_parts(upto, sizes):
    """f[n] = the fewest parts from ``sizes`` that add up to n, over ALL ways of writing n (dynamic programme)"""
    f = [0] + [None] * upto
    for n in range(1, upto + 1):
        f[n] = 1 + min(f[n - s] for s in sizes if s <= n)
    return f


def _c_loop(n, sizes):
    """the host loop as the C code runs it: one launch of the widest kernel that still fits, until nothing is left"""
    done, out = 0, []
    while done < n:
        left = n - done
        c = 1
        for s in sorted(sizes):
            if left >= s:
                c = s
        out.append(c)
        done += c
    return out


def test_split_plans_agree_with_brute_force():
    fr, fz = _fewest_parts(1100, (16, 8, 4, 2, 1)), _fewest_parts(1100, (8, 4, 2, 1))
    for n in range(1, 1101):
        r, z = pr.split_real(n), pr.split_c128(n)
        assert sum(r) == n and sum(z) == n
        assert r == sorted(r, reverse=True) and z == sorted(z, reverse=True)
        assert set(r) <= {16, 8, 4, 2, 1} and set(z) <= {8, 4, 2, 1}
        assert len(r) == n // 16 + bin(n % 16).count("1") and len(z) == n // 8 + bin(n % 8).count("1")
        assert len(r) == fr[n] and len(z) == fz[n], "no plan has fewer launches"
        assert r == _c_loop(n, (16, 8, 4, 2, 1)) and z == _c_loop(n, (8, 4, 2, 1)), n
        # dot_panel_dev: the launches tile [0, n) in order, none crosses an outer chunk, every partial slot is below MAXC
        at = 0
        for first, width in pr.dot_launches_real(n):
            assert first == at and first // pr.MAXC == (first + width - 1) // pr.MAXC and first % pr.MAXC + width <= pr.MAXC
            at += width
        assert at == n and sum(pr.outer_chunks(n)) == n and max(pr.outer_chunks(n)) <= pr.MAXC
        for cap in (pr.CAP, pr.ZCAP):
            calls = pr.wrapper_calls(n, cap)
            assert sum(calls) == n and max(calls) <= cap and all(c == cap for c in calls[:-1])
        assert sum(pr.passes(n, pr.KMAX)) == n and sum(pr.passes(n, pr.KP)) == n


# ---- the constants, read from the sources ----------------------------------------------------------------------------------------
def test_constants_are_what_the_sources_say():
    internal = _src("krypy_amd", "csrc", "kh_internal.h")
    steps = _src("krypy_amd", "csrc", "krylov_steps.h")
    zpath = _src("krypy_amd", "csrc", "zpath.h")
    main = _src("krypy_amd", "csrc", "krylov_hip.hip")
    assert _const(internal, "MAXC") == pr.MAXC and _const(zpath, "ZMAXC") == pr.ZMAXC and _const(internal, "BS") == pr.BS
    sc_coef, sc_ls, scal_cap = _const(steps, "SC_COEF"), _const(steps, "SC_LS"), _const(internal, "SCAL_CAP")
    assert _const(zpath, "ZSC_COEF") == sc_coef, "the complex entries stage their coefficients where the real ones do"
    assert _const(main, "KMAX") == pr.KMAX and _const(main, "KP") == pr.KP
    # the caps of the C entry points
    assert len(re.findall(r"KH_ARG\(ncols <= %d, \"kh_(?:dot|axpy)_panel" % pr.CAP, main)) == 2
    assert re.search(r"KH_ARG\(nx <= %d, \"kh_gemm_tn" % pr.CAP, main)
    assert len(re.findall(r"ncols <= %d, \"kh_z(?:dot|axpy)_panel" % pr.ZCAP, zpath)) == 2
    assert re.search(r"k <= %d && X != Y, \"kh_zgemm_nn" % pr.ZCAP, zpath)
    # the arithmetic the C code assumes: a full real call, a full pass and a full complex call (two doubles each) end at or
    # before SC_LS, where the one-reduction Gram-Schmidt keeps its scalars; nothing leaves the allocation
    assert sc_coef + pr.CAP <= sc_ls and sc_coef + pr.KMAX <= sc_ls
    assert 2 * pr.ZCAP <= sc_ls - sc_coef
    assert sc_ls <= scal_cap and pr.KP * 16 <= pr.CAP, "a pass of k_panel_gemm_mfma stages 64 x nc <= 1024 coefficients"
    assert 2 * pr.ZMAXC <= pr.MAXC, "a complex launch writes two partial slots per column into the real launches' slots"
    # the greedy rules themselves
    assert len(re.findall(r">= 16 \? 16 : \w+ >= 8 \? 8 : \w+ >= 4 \? 4 : \w+ >= 2 \? 2 : 1;", main)) == 2
    assert len(re.findall(r"left >= 8 \? 8 : left >= 4 \? 4 : left >= 2 \? 2 : 1;", zpath)) == 2
    assert re.search(r"std::min<int64_t>\(MAXC, ncols - done\)", main)
    assert re.search(r"const int b = \(done > 0\) \? 1 :", main) and re.search(r"const int b = \(done > 0\) \? 1 :", zpath)
    assert re.search(r"i0 == 0 \? beta : 1\.0", main)


def test_wrapper_strides_equal_the_c_caps():
    hip_py = _src("krypy_amd", "_hip.py")

    def body(name):
        m = re.search(r"    def %s\(self.*?(?=\n    def )" % name, hip_py, re.S)
        assert m, name
        return m.group(0)

    dot, axpy, nn, tn = body("dot_panel"), body("axpy_panel"), body("gemm_nn"), body("gemm_tn")
    for text in (dot, axpy):
        assert re.search(r"range\(0, max\(ncols, 1\), %d\)" % pr.ZCAP, text) and re.search(r"min\(%d, ncols - c0\)" % pr.ZCAP, text)
        assert re.search(r"range\(0, max\(ncols, 1\), %d\)" % pr.CAP, text) and re.search(r"min\(%d, ncols - c0\)" % pr.CAP, text)
    assert re.search(r"min\(%d, k - done\)" % pr.ZCAP, nn) and "done, b = done + m, 1.0" in nn
    assert re.search(r"range\(0, nx, %d\)" % pr.CAP, tn) and re.search(r"min\(%d, nx - r0\)" % pr.CAP, tn)
    assert re.search(r"min\(%d, nx - done\)" % pr.ZCAP, tn)


def test_grids_and_chain_lengths():
    """the grid formulas at the sizes the GPU tests use, and the chain lengths they give (worked by hand from kernels.h)"""
    assert pr.grid_for(1, 1024) == 1 and pr.grid_for(513, 1024) == 1 and pr.grid_for(514, 1024) == 2
    assert pr.grid_for(100003, 1024) == 196 and pr.grid_for(100003, 3) == 3 and pr.grid_lin(100003, 3) == 6
    assert pr.zgrid(4097, 1024) == 17 and pr.zgrid(4097, 1) == 1
    # n = 100003 on one workgroup: 50001 double2 elements over 256 lanes = 196 trips of two fmas, the odd element, the tree,
    # one partial added to 0.0 and the tree again, the reference
    assert pr.chain_dot(100003, 1) == 2 * 196 + 1 + 9 + (1 + 9) + 1
    assert pr.chain_dot(1, 1024) == 0 + 1 + 9 + 10 + 1 and pr.chain_dot(2, 1024) == 2 + 0 + 9 + 10 + 1
    assert pr.chain_zdot(4097, 3) == 2 * 6 + 9 + 10 + 1
    assert pr.chain_cg(100003, 3, True) == 66 + 9 + 10 + 1 + 1
    assert pr.chain_panel_gemm(1100) == 1100 + 18 + 3
    assert pr.gamma(pr.chain_dot(100003, 1)) < 5e-14


# ---- order-exact against extended ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: "%s-%d" % (c.path, c.width))
def test_folds_agree_with_longdouble(case):
    """w - sum h_c v_c, left to right with two roundings per column, against the longdouble value: gamma(2 k + 1) of the
    absolute terms (k products, k subtractions, the rounding of sign * coef - an exact sign flip here)."""
    n, k = 5, case.width
    cplx = case.path == "c128"
    V, w, h = pc.block(n, k, 7 * k, cplx), pc.block(n, 1, 7 * k + 1, cplx)[:, 0], pc.coefficients(k, 7 * k + 2, cplx)
    bar = pr.gamma(2 * k + 2)
    if not cplx:
        got = pr.fold_real(w, V, h, 1.0, 1.0)
        terms = V.astype(LD) * h.astype(LD)[None, :]
        want, mag = w.astype(LD) - terms.sum(axis=1), np.abs(w) + np.abs(terms).sum(axis=1)
        assert np.all(np.abs(got.astype(LD) - want) <= bar * mag)
        assert np.array_equal(pr.fold_real(w, V, -h, -1.0, 1.0), got), "an exact sign flip"
        half = pr.fold_real(pr.fold_real(w, V[:, :k // 2], h[:k // 2], 1.0, 1.0), V[:, k // 2:], h[k // 2:], 1.0, 1.0)
        assert np.array_equal(half, got), "the fold does not depend on where it is cut"
        return
    gr, gi = pr.fold_c128(w.real, w.imag, V.real.copy(), V.imag.copy(), h.real, h.imag, 1.0, 1.0)
    Vl, hl = V.real.astype(LD) + 1j * V.imag.astype(LD), h.real.astype(LD) + 1j * h.imag.astype(LD)
    want = (w.real.astype(LD) + 1j * w.imag.astype(LD)) - (Vl * hl[None, :]).sum(axis=1)
    mag = np.abs(w) + (np.abs(V) * np.abs(h)[None, :]).sum(axis=1)
    assert np.all(np.abs((gr.astype(LD) + 1j * gi.astype(LD)) - want) <= 2 * pr.gamma(2 * k + 3) * mag)


def test_beta_forms_and_the_gemm_references():
    n, k = 9, 37
    X, C, Y = pc.block(n, k, 1), pc.coefficients(k * 3, 2).reshape(k, 3), pc.block(n, 3, 3)
    nan = np.full_like(Y, np.nan)
    for alpha, beta in pc.GEMM_AB:
        got = pr.gemm_nn_real(X, C, alpha, beta, nan if beta == 0.0 else Y)
        assert np.all(np.isfinite(got)), "beta == 0 reads nothing"
        want, mag = pr.gemm_nn_ld(X, C, alpha, beta, Y)
        assert np.all(np.abs(got.astype(LD) - want) <= pr.gamma(2 * k + 3) * mag)
        one = np.stack([pr.gemm_nn_real(X, C[:, c], alpha, beta, (nan if beta == 0.0 else Y)[:, c]) for c in range(3)], axis=1)
        assert np.array_equal(one.reshape(n, 3), got), "the columns of the block form are independent folds"
    empty = X[:, :0]
    assert np.array_equal(pr.gemm_nn_real(empty, C[:0], 1.0, 0.0, nan), np.zeros_like(Y))
    assert np.array_equal(pr.gemm_nn_real(empty, C[:0], 1.0, 1.0, Y), Y)
    assert np.array_equal(pr.gemm_nn_real(empty, C[:0], 2.0, 0.5, Y), 0.5 * Y)
    Z, zc, zy = pc.block(n, k, 4, True), pc.coefficients(k, 5, True), pc.block(n, 1, 6, True)
    alpha = 0.75 - 0.5j
    for beta in pc.ZGEMM_BETA:
        yr, yi = (np.full(n, np.nan),) * 2 if beta == 0.0 else (zy[:, 0].real, zy[:, 0].imag)
        gr, gi = pr.gemm_nn_c128(Z.real.copy(), Z.imag.copy(), zc, alpha, beta, yr, yi)
        want = beta * zy[:, 0] + Z.dot(zc * alpha)
        mag = abs(beta) * np.abs(zy[:, 0]) + np.abs(Z).dot(np.abs(zc * alpha))
        assert np.all(np.abs((gr + 1j * gi) - want) <= 64 * k * pr.U * mag)
    er, ei = pr.gemm_nn_c128(Z.real[:, :0], Z.imag[:, :0], zc[:0], alpha, 0.5, zy[:, 0].real, zy[:, 0].imag)
    assert np.array_equal(er + 1j * ei, 0.5 * zy[:, 0]), "k == 0 scales Y"


def test_complex_product_rounds_every_operation():
    """cmul is the DEVICE's product (four products and two sums, each rounded): within two roundings of the exact one.  The
    host's C * alpha inside Context.gemm_nn is NumPy's, which may be fused - the reference takes that one from NumPy."""
    c, alpha = pc.coefficients(1025, 11, True), 0.75 - 0.5j
    re, im = pr.cmul(c.real.copy(), c.imag.copy(), np.float64(alpha.real), np.float64(alpha.imag))
    cr, ci, ar, ai = c.real.astype(LD), c.imag.astype(LD), LD(alpha.real), LD(alpha.imag)
    assert np.all(np.abs(re.astype(LD) - (cr * ar - ci * ai)) <= pr.gamma(3) * (np.abs(cr * ar) + np.abs(ci * ai)))
    assert np.all(np.abs(im.astype(LD) - (cr * ai + ci * ar)) <= pr.gamma(3) * (np.abs(cr * ai) + np.abs(ci * ar)))
    assert np.allclose(re + 1j * im, c * alpha, rtol=4 * pr.U, atol=0)


def test_streaming_references():
    n = 11
    x, y = pc.block(n, 1, 21)[:, 0], pc.block(n, 1, 22)[:, 0]
    nan = np.full(n, np.nan)
    assert np.array_equal(pr.waxpby(1.0, x, 0.0, nan), x) and np.array_equal(pr.waxpby(1.0, x, 1.0, y), x + y)
    assert np.array_equal(pr.waxpby(-2.5, x, 0.75, y), (-2.5 * x) + (0.75 * y))
    assert np.array_equal(pr.waxpby(0.5, x, 0.0, nan), 0.5 * x)
    z = pc.block(n, 2, 23, True)
    a, b = 0.5 + 0.25j, -1.5 + 2.0j
    rr, ri = pr.zwaxpby(a, z[:, 0].real, z[:, 0].imag, b, z[:, 1].real, z[:, 1].imag)
    assert np.allclose(rr + 1j * ri, a * z[:, 0] + b * z[:, 1], rtol=1e-15, atol=0)
    rr, ri = pr.zwaxpby(a, z[:, 0].real, z[:, 0].imag, 0j, nan, nan)
    assert np.array_equal(rr + 1j * ri, a * z[:, 0])
    zz, yk = pr.minres_update(x, y, x * y, 0.5, -0.25, 1.75, 0.375, y)
    assert np.array_equal(zz, ((x - 0.5 * y) - (-0.25) * (x * y)) / 1.75) and np.array_equal(yk, y + 0.375 * zz)
    yk, r, zv = pr.cg_update(0.40625, x, y, x, y, np.abs(x))
    assert np.array_equal(yk, x + 0.40625 * x) and np.array_equal(r, y - 0.40625 * y) and np.array_equal(zv, np.abs(x) * r)
    v, s = pr.dot_ld(np.stack([x, y], axis=1), y)
    assert abs(float(v[0]) - x.dot(y)) <= pr.gamma(n) * float(s[0]) and s[1] == v[1]
    re, im, are, aim = pr.zdot_ld(z[:, :1].real, z[:, :1].imag, z[:, 1].real, z[:, 1].imag)
    want = np.vdot(z[:, 0], z[:, 1])
    assert abs(complex(re[0], im[0]) - want) <= pr.gamma(2 * n) * float(are[0] + aim[0]), "conj on the LEFT argument"


def test_numpy_context_scales_y_when_there_is_no_column(cpu_double):
    """Y = beta Y + X C with k == 0 (kh_gemm_nn, kh_zgemm_nn): the CPU double follows the rule the device entries follow."""
    for cplx in (False, True):
        y0 = pc.block(6, 3, 31, cplx)
        X = cpu_double.upload(pc.block(6, 2, 32, cplx))
        for beta, want in ((0.5, 0.5 * y0[:, 1]), (1.0, y0[:, 1]), (0.0, 0 * y0[:, 1])):
            Y = cpu_double.upload(y0)
            cpu_double.gemm_nn(X, 0, 0, np.zeros((0, 1)), 1.0, beta, Y, 1)
            got = Y.download()
            assert np.array_equal(got[:, 1], want) and np.array_equal(got[:, [0, 2]], y0[:, [0, 2]])
