"""GPU tests of the Chebyshev polynomial preconditioner (krypy_amd/csrc/cheb.hip, EPI_CHEB in kernels.h): the device result must
be the oracle's array expressions (tests/support/cheb_ref.py) bit for bit - fused and composed, banded and CSR-stream -, the
storage contracts hold, and a solver preconditioned with the device operator must produce the bits of the same solver with a
host-callable twin."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import cheb_cases as cc
from tests.support.cheb_ref import cheb_apply_ref, cheb_coefficients
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal, poison, poisoned_allocations

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"      # a 1-rank communicator: the composed path serves
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4099, 70001]
DEGREES = [1, 2, 5]


@pytest.fixture
def switches(hip):
    """Whatever a test sets, the library's defaults are back afterwards."""
    keys = ("cheb_fused", "spmv_dia", "spmv_win")
    before = {k: hip.get(k) for k in keys}
    yield hip
    for k, v in before.items():
        hip.set(k, v)


def _rhs(n, ncols=1, seed=0, cplx=False):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, ncols))
    return b + 1j * rng.standard_normal((n, ncols)) if cplx else b


def _apply(ctx, dm, dinv, coef, b):
    """(result, fused launches, update launches, mask-form launches) of one kh_cheb_apply on fresh blocks."""
    X = ctx.upload(b, dtype=dm.dtype)
    Y = ctx.alloc(X.n, X.ncols, dtype=dm.dtype, zero=False)
    S = ctx.alloc(X.n, 3, dtype=dm.dtype, zero=False)
    D = None if dinv is None else ctx.diag(np.repeat(dinv, 2) if dm.dtype.kind == "c" else dinv)
    c0 = [ctx.get(k) for k in ("n_cheb_fused", "n_cheb_update", "n_dia_mask", "n_cheb_apply")]
    ctx.cheb_apply(dm, D, coef, X, 0, Y, 0, X.ncols, S)
    c1 = [ctx.get(k) for k in ("n_cheb_fused", "n_cheb_update", "n_dia_mask", "n_cheb_apply")]
    return (Y.download(),) + tuple(b1 - b0 for b0, b1 in zip(c0, c1))


def _check_paths(ctx, A, kind, n):
    """Every degree, with and without scaling, on every path the operator has: the oracle's bits, and the counters say which
    path ran."""
    dm = ctx.csr(A)
    lmax = cc.gershgorin_lmax(A)
    b = _rhs(n, 1, seed=n)
    b[0, 0] = -0.0 if n > 1 else b[0, 0]                       # step 0 stores d itself as z: -0.0 stays -0.0 at degree 1
    scale = np.random.default_rng(n + 1).uniform(0.5, 2.0, n)
    configs = [dict(cheb_fused=1), dict(cheb_fused=0)]
    if kind in ("mask", "value"):
        configs += [dict(cheb_fused=1, spmv_dia=0), dict(cheb_fused=0, spmv_dia=0)]
    else:
        configs += [dict(cheb_fused=1, spmv_win=0)]
    for m in DEGREES:
        for dinv in (None, 1.0 / scale):
            coef = cheb_coefficients(lmax / 30.0, lmax * (2.0 if dinv is not None else 1.0), m)
            want = cheb_apply_ref(A, b, coef, dinv)
            for cfg in configs:
                for k, v in dict(dict(cheb_fused=1, spmv_dia=1, spmv_win=1), **cfg).items():
                    ctx.set(k, v)
                got, fused, upd, mask, applied = _apply(ctx, dm, dinv, coef, b)
                what = "%s n=%d m=%d scaled=%s %s" % (kind, n, m, dinv is not None, cfg)
                bits_equal(got, want, what)
                on = cfg["cheb_fused"] == 1 and not FORCED
                expect_kernel(applied == 1, "%s: n_cheb_apply moved by %d" % (what, applied))
                expect_kernel(fused == (m - 1 if on else 0), "%s: %d fused launches" % (what, fused))
                expect_kernel(upd == (1 if on else m), "%s: %d update launches" % (what, upd))
                if kind == "mask" and n >= 3 and cfg.get("spmv_dia", 1) == 1:
                    expect_kernel(mask == m - 1, "%s: n_dia_mask moved by %d" % (what, mask))
                if kind == "value" or cfg.get("spmv_dia", 1) == 0:
                    expect_kernel(mask == 0, "%s: n_dia_mask moved by %d" % (what, mask))


@pytest.mark.parametrize("n", SIZES)
def test_oracle_bits_mask_form(switches, n):
    """The 1-D three-point Laplacian: constant coefficients, the banded kernel's mask form."""
    A = cc.lap1d(n)
    dm = switches.csr(A)
    expect_kernel(n < 3 or dm.diagonals == 3, "lap1d(%d) has no banded form (%d diagonals)" % (n, dm.diagonals))
    _check_paths(switches, A, "mask", n)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_bits_value_form(switches, n):
    """The same with a varying diagonal: the banded kernel's value form."""
    _check_paths(switches, cc.lap1d(n, vary=True), "value", n)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_bits_csr_stream(switches, n):
    """A seeded random symmetric diagonally dominant matrix of ~7 entries per row: the CSR-stream kernel, with and without
    its LDS window."""
    A = cc.random_spd(n, 7, seed=n)
    dm = switches.csr(A)
    expect_kernel(n < 64 or dm.diagonals == 0, "random_spd(%d) got a banded form" % n)
    _check_paths(switches, A, "stream", n)


def test_many_steps_write_their_records_in_chunks(switches):
    """Degree 40: more fused steps than one launch writes records for."""
    n, m = 2049, 40
    A = cc.lap1d(n)
    coef = cheb_coefficients(4.0 / 30.0, 4.0, m)
    b = _rhs(n, 2, seed=40)
    got, fused, upd, _, applied = _apply(switches, switches.csr(A), None, coef, b)
    bits_equal(got, cheb_apply_ref(A, b, coef), "degree 40")
    expect_kernel(fused == (0 if FORCED else 2 * (m - 1)) and applied == 2, "degree 40: %d fused launches, %d columns" % (fused, applied))


@pytest.mark.parametrize("nx,ny", [(37, 23), (300, 200)])
def test_oracle_bits_five_point_laplacian(switches, nx, ny):
    A = cc.lap2d(nx, ny)
    n = nx * ny
    dm = switches.csr(A)
    expect_kernel(dm.diagonals == 5, "lap2d has %d diagonals" % dm.diagonals)
    coef = cheb_coefficients(8.0 / 30.0, 8.0, 4)
    b = _rhs(n, 1, seed=nx)
    dinv = 1.0 / np.random.default_rng(ny).uniform(0.5, 2.0, n)
    for sc in (None, dinv):
        want = cheb_apply_ref(A, b, coef, sc)
        for on in (1, 0):
            switches.set("cheb_fused", on)
            got, fused, _, mask, _ = _apply(switches, dm, sc, coef, b)
            bits_equal(got, want, "lap2d %dx%d fused=%d scaled=%s" % (nx, ny, on, sc is not None))
            expect_kernel(fused == (3 if on and not FORCED else 0), "lap2d: %d fused launches" % fused)
            expect_kernel(mask == 3, "lap2d: n_dia_mask moved by %d" % mask)


def test_row_longer_than_the_tile(switches):
    """A dense first row at n = 4099 takes the kernel's long-row branch (a tree sum): fused equals composed bit for bit, and
    the oracle at 1e-12."""
    n = 4099
    A = cc.random_spd(n, 7, seed=9).tolil()
    A[0, 1:] = 1e-3
    A[1:, 0] = 1e-3
    A[0, 0] = A[0, 0] + 5.0
    A = A.tocsr()
    A.sort_indices()
    dm = switches.csr(A)
    lmax = cc.gershgorin_lmax(A)
    coef = cheb_coefficients(lmax / 30.0, lmax, 5)
    b = _rhs(n, 1, seed=5)
    dinv = 1.0 / A.diagonal()
    for sc in (None, dinv):
        switches.set("cheb_fused", 1)
        got_f, fused, _, _, _ = _apply(switches, dm, sc, coef, b)
        switches.set("cheb_fused", 0)
        got_c, none, _, _, _ = _apply(switches, dm, sc, coef, b)
        bits_equal(got_f, got_c, "long row, fused against composed")
        want = cheb_apply_ref(A, b, coef, sc)
        assert np.linalg.norm(got_f - want) <= 1e-12 * np.linalg.norm(want)
        expect_kernel(fused == (0 if FORCED else 4) and none == 0, "long row: %d / %d fused launches" % (fused, none))


@pytest.mark.parametrize("kind,n", [("mask", 4099), ("stream", 2049), ("dense", 65)])
@pytest.mark.parametrize("fused", [1, 0])
def test_storage_contracts(switches, kind, n, fused):
    """Poisoned scratch and Y: the same bits, the padding stays zero, two calls are bit-identical (ncols = 3, distinct columns)."""
    A = cc.lap1d(n) if kind == "mask" else cc.random_spd(n, 7, seed=1)
    ctx = switches
    ctx.set("cheb_fused", fused)
    dm = ctx.dense(A.toarray()) if kind == "dense" else ctx.csr(A)
    lmax = cc.gershgorin_lmax(A)
    coef = cheb_coefficients(lmax / 30.0, lmax, 4)
    b = _rhs(n, 3, seed=2)
    dinv = 1.0 / A.diagonal()
    want = cheb_apply_ref(A, b, coef, dinv)
    with poisoned_allocations(ctx):
        X = ctx.upload(b)
        D = ctx.diag(dinv)
        Y = ctx.alloc(n, 5, zero=False)
        S = ctx.alloc(n, 3, zero=False)
        out = []
        for _ in range(2):
            poison(Y)
            poison(S)
            ctx.cheb_apply(dm, D, coef, X, 0, Y, 1, 3, S)
            out.append(Y.download(1, 3))
            assert not Y.padding_nonzero() and not S.padding_nonzero() and not X.padding_nonzero()
            assert np.all(np.isnan(Y.download(0, 1))) and np.all(np.isnan(Y.download(4, 1)))     # the neighbours are not written
        bits_equal(X.download(), b, "x is only read")
    if kind == "dense":
        assert np.linalg.norm(out[0] - want) <= 1e-13 * np.linalg.norm(want)      # (the dense kernel sums in another order)
    else:
        bits_equal(out[0], want, "poisoned blocks, %s fused=%d" % (kind, fused))
    bits_equal(out[0], out[1], "two calls")


def test_cheb_update_alone(switches):
    """The composed step on its own: step 0 reads neither d nor z, a later step may update z in place."""
    ctx = switches
    n = 2049
    A = cc.lap1d(n)
    coef = cheb_coefficients(0.1, 4.0, 3)
    b = _rhs(n, 1, seed=6)
    dinv = np.random.default_rng(7).uniform(0.5, 2.0, n)
    X, D = ctx.upload(b), ctx.diag(dinv)
    W = poison(ctx.alloc(n, 3, zero=False))            # d, z, A z
    dm = ctx.csr(A)
    ctx.cheb_update(None, 0, X, 0, D, W, 0, None, 0, W, 1, 0.0, coef[0, 1], first=True)
    for k in (1, 2):
        ctx.apply(dm, W, 1, W, 2, 1)
        ctx.cheb_update(W, 2, X, 0, D, W, 0, W, 1, W, 1, coef[k, 0], coef[k, 1])
    bits_equal(W.download(1, 1), cheb_apply_ref(A, b, coef, dinv), "three composed steps, z in place")
    assert not W.padding_nonzero()


def test_argument_errors(switches):
    from krypy_amd._hip import BackendError

    ctx = switches
    n = 130
    A = ctx.csr(cc.lap1d(n))
    Z = ctx.csr(cc.lap1d(n).astype(complex))
    coef = cheb_coefficients(0.1, 4.0, 3)
    X, Y, S = ctx.alloc(n, 4), ctx.alloc(n, 4), ctx.alloc(n, 3)
    Xc, Yc, Sc = (ctx.alloc(n, k, dtype=complex) for k in (2, 2, 3))
    ctx.cheb_apply(A, None, coef, X, 0, X, 2, 2, S)                   # one block, disjoint columns: fine
    bad = [
        ("overlap", lambda: ctx.cheb_apply(A, None, coef, X, 0, X, 0, 1, S)),
        ("overlap", lambda: ctx.cheb_apply(A, None, coef, X, 0, X, 1, 2, S)),
        ("scratch", lambda: ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, ctx.alloc(n, 1))),
        ("scratch", lambda: ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, X)),
        ("scratch", lambda: ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, Y)),
        ("length|expected", lambda: ctx.cheb_apply(A, None, coef, ctx.alloc(n + 1, 1), 0, Y, 0, 1, S)),
        ("length|expected", lambda: ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, ctx.alloc(n - 1, 3))),
        ("out of range", lambda: ctx.cheb_apply(A, None, coef, X, 3, Y, 0, 2, S)),
        ("operator on", lambda: ctx.cheb_apply(A, None, coef, Xc, 0, Yc, 0, 1, Sc)),
        ("operator on", lambda: ctx.cheb_apply(Z, None, coef, X, 0, Y, 0, 1, S)),
        ("mixed", lambda: ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, Sc)),
        ("Dinv", lambda: ctx.cheb_apply(A, A, coef, X, 0, Y, 0, 1, S)),
        ("Dinv", lambda: ctx.cheb_apply(A, ctx.diag(np.ones(n + 1)), coef, X, 0, Y, 0, 1, S)),
        ("Dinv", lambda: ctx.cheb_apply(Z, ctx.diag(np.ones(n)), coef, Xc, 0, Yc, 0, 1, Sc)),      # 2 n entries for a complex block
        ("Dinv", lambda: ctx.cheb_apply(A, ctx.diag(np.ones(n, dtype=complex)), coef, X, 0, Y, 0, 1, S)),
        ("diagonal", lambda: ctx.cheb_apply(ctx.diag(np.ones(n)), None, coef, X, 0, Y, 0, 1, S)),
        ("coefficients", lambda: ctx.cheb_apply(A, None, np.zeros(4), X, 0, Y, 0, 1, S)),
        ("degree", lambda: ctx.cheb_apply(A, None, np.zeros((0, 2)), X, 0, Y, 0, 1, S)),
        # kh_cheb_update
        ("different columns", lambda: ctx.cheb_update(None, 0, X, 0, None, X, 0, None, 0, Y, 0, 0.0, 1.0, first=True)),
        ("different columns", lambda: ctx.cheb_update(None, 0, X, 0, None, Y, 0, None, 0, Y, 0, 0.0, 1.0, first=True)),
        ("differ", lambda: ctx.cheb_update(S, 0, X, 0, None, S, 0, Y, 0, Y, 0, 1.0, 1.0)),
        ("differ", lambda: ctx.cheb_update(S, 1, X, 0, None, S, 0, S, 0, Y, 0, 1.0, 1.0)),
        ("expected", lambda: ctx.cheb_update(S, 1, X, 0, None, S, 0, Y, 0, ctx.alloc(n + 2, 1), 0, 1.0, 1.0)),
        ("mixed", lambda: ctx.cheb_update(S, 1, X, 0, None, S, 0, Yc, 0, Y, 0, 1.0, 1.0)),
        ("Dinv", lambda: ctx.cheb_update(S, 1, X, 0, A, S, 0, Y, 0, Y, 0, 1.0, 1.0)),
        ("Dinv", lambda: ctx.cheb_update(S, 1, X, 0, ctx.diag(np.ones(n - 1)), S, 0, Y, 0, Y, 0, 1.0, 1.0)),
        ("NULL", lambda: ctx.cheb_update(None, 1, X, 0, None, S, 0, Y, 0, Y, 0, 1.0, 1.0)),
    ]
    for pattern, call in bad:
        with pytest.raises(BackendError, match=pattern):
            call()


@pytest.mark.parametrize("scaled", [False, True])
def test_complex_hermitian_operator(switches, scaled):
    """A Hermitian positive definite c128 matrix: the composed path, the oracle's bits."""
    from krypy_amd import utils

    A = cc.hermitian_perturbed(37, 23)
    n = A.shape[0]
    assert abs(A - A.conj().T).max() == 0 and np.linalg.eigvalsh(A.toarray()).min() > 0
    s = np.random.default_rng(12).uniform(0.5, 2.0, n) if scaled else None
    op = utils.ChebyshevOperator(A, cc.gershgorin_lmax(A) * (2.0 if scaled else 1.0), degree=4, scale=s)
    b = _rhs(n, 2, seed=13, cplx=True)
    f0, u0 = switches.get("n_cheb_fused"), switches.get("n_cheb_update")
    got = op.dot(b)
    fused, upd = switches.get("n_cheb_fused") - f0, switches.get("n_cheb_update") - u0
    bits_equal(got, cheb_apply_ref(A, b, op.coefficients, None if s is None else 1.0 / s), "complex operator")
    expect_kernel(fused == 0 and upd == 8, "complex: %d fused launches, %d updates" % (fused, upd))


@pytest.mark.parametrize("scaled", [False, True])
def test_generic_operator_path(hip, scaled):
    """A as a product of two operators (B * B, B the shifted 1-D Laplacian): one ``A._apply_dev`` and one ``cheb_update`` per
    step; the oracle's bits with the product formed the same way, B (B z)."""
    from krypy_amd import utils

    n = 4099
    B = (cc.lap1d(n) + sp.identity(n)).tocsr()

    class BB(object):
        dtype = np.dtype(float)

        @staticmethod
        def dot(z):
            return B.dot(B.dot(z))

    s = np.random.default_rng(14).uniform(0.5, 2.0, n) if scaled else None
    op = utils.ChebyshevOperator(utils.MatrixLinearOperator(B) * utils.MatrixLinearOperator(B), 25.0 * (2.0 if scaled else 1.0),
                                 degree=5, scale=s)
    b = _rhs(n, 2, seed=15)
    c0 = [hip.get(k) for k in ("n_cheb_update", "n_cheb_apply", "n_cheb_fused")]
    got = op.dot(b)
    c1 = [hip.get(k) for k in ("n_cheb_update", "n_cheb_apply", "n_cheb_fused")]
    bits_equal(got, cheb_apply_ref(BB, b, op.coefficients, None if s is None else 1.0 / s), "generic operator")
    expect_kernel([y - x for x, y in zip(c0, c1)] == [10, 0, 0], "generic path: counters moved by %s" % [y - x for x, y in zip(c0, c1)])


# ---- solvers -----------------------------------------------------------------------------------------------------------------
class _Twin(object):
    """The oracle as a host callable, every application counted."""

    def __init__(self, A, coef, dinv=None):
        from krypy_amd import utils

        self.calls = 0
        n = A.shape[0]

        def dot(X):
            self.calls += X.shape[1]
            return cheb_apply_ref(A, X, coef, dinv)

        self.op = utils.LinearOperator((n, n), float, dot=dot)


def _run(solver, A, b, maxiter, **prec):
    from krypy_amd import linsys, utils

    ls = linsys.LinearSystem(A, b, **prec)
    try:
        sol = solver(ls, tol=1e-9, maxiter=maxiter)
    except utils.ConvergenceError as e:
        sol = e.solver
    return np.array(sol.resnorms), np.array(sol.xk)


@pytest.mark.parametrize("nx,ny,maxiter", [(37, 23, 80), (300, 200, 3)])
@pytest.mark.parametrize("solver,key", [("Cg", "M"), ("Minres", "M"), ("Gmres", "M"), ("Gmres", "Ml")])
def test_solvers_against_host_callable_twins(hip, solver, key, nx, ny, maxiter):
    from krypy_amd import linsys, utils

    A = cc.lap2d(nx, ny)
    b = _rhs(nx * ny, 1, seed=21)
    op = utils.ChebyshevOperator(A, 8.0, degree=4)
    twin = _Twin(A, op.coefficients)
    flags = dict(self_adjoint=True, positive_definite=True) if key == "M" else {}
    s0 = hip.get("n_cheb_apply")
    res_d, x_d = _run(getattr(linsys, solver), A, b, maxiter, **dict(flags, **{key: op}))
    applied = hip.get("n_cheb_apply") - s0
    res_t, x_t = _run(getattr(linsys, solver), A, b, maxiter, **dict(flags, **{key: twin.op}))
    bits_equal(res_d, res_t, "resnorms")
    bits_equal(x_d, x_t, "xk")
    assert applied == twin.calls and applied >= len(res_d) - 1
    assert hip.get("n_cheb_apply") - s0 == applied          # the twin's run never touched the kernels
    if maxiter > 3:
        assert res_d[-1] <= 1e-9 and len(res_d) - 1 < maxiter
    else:
        assert len(res_d) - 1 == 3 and res_d[-1] < res_d[0]


def test_cg_needs_at_most_half_the_iterations(hip):
    """37 x 23, ``chebyshev_operator(A, degree=4)``: 33 iterations against 115 on the CPU double."""
    from krypy_amd import linsys, utils

    A = cc.lap2d(37, 23)
    b = _rhs(37 * 23, 1, seed=22)
    plain, _ = _run(linsys.Cg, A, b, 400, self_adjoint=True, positive_definite=True)
    op = utils.chebyshev_operator(A, degree=4)
    assert 7.9 < op.lmax <= 1.1 * 8.0
    pre, _ = _run(linsys.Cg, A, b, 400, M=op, self_adjoint=True, positive_definite=True)
    print("CG iterations: plain %d, Chebyshev degree 4 %d" % (len(plain) - 1, len(pre) - 1))
    assert plain[-1] <= 1e-9 and pre[-1] <= 1e-9
    assert 2 * (len(pre) - 1) <= len(plain) - 1


@pytest.mark.parametrize("solver", ["Cg", "Minres", "Gmres"])
def test_against_recorded_reference(hip, golden, solver):
    """The unmodified reference's solvers with ``M = LinearOperator(dot=oracle)`` on the 24 x 17 Laplacian
    (tools/gen_cheb_golden.py; lmax = 8.8, ratio 30, degree 4, tol 1e-9).  resnorms[:-1] at 1e-10 relative (the reference's own
    sensitivity to one-ulp noise in M is 1e-14 there); the last entry is an explicitly formed residual and moves by 1e-7
    relative: 1e-10 * resnorms[0] absolute."""
    from krypy_amd import linsys, utils

    g = golden("cheb_precond")
    n = int(g["n"])
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(n, n))
    op = utils.ChebyshevOperator(A, float(g["lmax"]), ratio=float(g["ratio"]), degree=int(g["degree"]))
    bits_equal(op.coefficients, g["coef"], "coefficients")
    sol = getattr(linsys, solver)(linsys.LinearSystem(A, g["b"], M=op, self_adjoint=True, positive_definite=True), tol=1e-9)
    got, want, xk = np.array(sol.resnorms), g["resnorms_" + solver.lower()], g["xk_" + solver.lower()]
    assert got.shape == want.shape
    assert np.max(np.abs(got[:-1] - want[:-1]) / want[:-1]) < 1e-10
    assert abs(got[-1] - want[-1]) <= 1e-10 * want[0]
    assert np.linalg.norm(sol.xk - xk) <= 1e-10 * np.linalg.norm(xk)


@pytest.mark.parametrize("mode", ["1", "2"])
def test_banded_measurement_modes(hip, mode):
    """KRYPY_AMD_SPMV_DIA is read once per process: the fused epilogue with 1 and 2 row pairs per lane is checked in a child
    process (as tests/test_gpu_parity.py does for the plain product) - the oracle's bits in both forms."""
    import subprocess
    import sys
    code = (
        "import numpy as np\n"
        "from krypy_amd import _hip\n"
        "from tests.support import cheb_cases as cc\n"
        "from tests.support.cheb_ref import cheb_apply_ref, cheb_coefficients\n"
        "from tests.support.poison import bits_equal\n"
        "ctx = _hip.get_context()\n"
        "for A in (cc.lap1d(65), cc.lap1d(4099), cc.lap1d(2049, vary=True), cc.lap2d(37, 23), cc.lap2d(97, 53)):\n"
        "    n = A.shape[0]\n"
        "    dm = ctx.csr(A)\n"
        "    assert dm.diagonals in (3, 5)\n"
        "    b = np.random.default_rng(n).standard_normal((n, 1))\n"
        "    dinv = 1.0 / np.random.default_rng(1).uniform(0.5, 2.0, n)\n"
        "    coef = cheb_coefficients(0.3, 16.0, 3)\n"
        "    X, Y, S, D = ctx.upload(b), ctx.alloc(n, 1), ctx.alloc(n, 3), ctx.diag(dinv)\n"
        "    f0 = ctx.get('n_cheb_fused')\n"
        "    ctx.cheb_apply(dm, D, coef, X, 0, Y, 0, 1, S)\n"
        "    bits_equal(Y.download(), cheb_apply_ref(A, b, coef, dinv), 'n = %d' % n)\n"
        "    assert ctx.get('n_cheb_fused') - f0 == 2 and not Y.padding_nonzero() and not S.padding_nonzero()\n"
        "print('ok')\n")
    env = dict(os.environ, KRYPY_AMD_SPMV_DIA=mode)
    env.pop("KRYPY_AMD_TEST_FORCE_MULTI", None)
    env.pop("KRYPY_AMD_FORCE_MULTI", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]
