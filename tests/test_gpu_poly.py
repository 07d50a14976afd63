"""GPU tests of the GMRES polynomial preconditioner (krypy_amd/csrc/poly.hip, EPI_POLY in kernels.h): the device result must be
the oracle's array expressions (tests/support/poly_ref.py) bit for bit - fused and composed, banded and CSR-stream -, the
storage contracts hold, the roots from the device's Arnoldi steps are the oracle's, and a solver preconditioned with the device
operator must produce the bits of the same solver with a host-callable twin.  The shared cases are those of
tests/test_poly_host.py."""
import itertools
import os

import numpy as np
import pytest

from tests.support import bicgstab_cases as bc
from tests.support import poly_cases as pc
from tests.support import poly_ref as ref
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal, poison, poisoned_allocations

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"      # a 1-rank communicator: the composed path serves
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4099, 70001]
COUNTERS = ("n_poly_fused", "n_poly_update", "n_dia_mask", "n_poly_apply")
CONFIGS = [dict(poly_fused=f, spmv_dia=d, spmv_win=w) for f, d, w in itertools.product((1, 0), (1, 0), (1, 0))]


@pytest.fixture
def switches(hip):
    """Whatever a test sets, the library's defaults are back afterwards."""
    keys = ("poly_fused", "spmv_dia", "spmv_win")
    before = {k: hip.get(k) for k in keys}
    yield hip
    for k, v in before.items():
        hip.set(k, v)


def _rhs(n, ncols=1, seed=0):
    return np.random.default_rng(seed).standard_normal((n, ncols))


def _apply(ctx, dm, steps, b):
    """(result, fused launches, update launches, mask-form launches, columns) of one kh_poly_apply on fresh, unwritten blocks."""
    X = ctx.upload(b)
    Y = ctx.alloc(X.n, X.ncols, zero=False)
    S = ctx.alloc(X.n, 3, zero=False)
    c0 = [ctx.get(k) for k in COUNTERS]
    ctx.poly_apply(dm, steps, X, 0, Y, 0, X.ncols, S)
    c1 = [ctx.get(k) for k in COUNTERS]
    return (Y.download(),) + tuple(b1 - b0 for b0, b1 in zip(c0, c1))


def _check_paths(ctx, A, kind, n):
    """Every table on every path the operator has: the oracle's bits, and - judged after the numbers - the counters say which
    path ran."""
    dm = ctx.csr(A)
    b = _rhs(n, 1, seed=n)
    b[0, 0] = -0.0
    for name in pc.ROOTS:
        steps = pc.table(name)
        nsteps = steps.shape[0]
        scale = int(steps[0, 0]) == 3
        want = ref.poly_apply_ref(A, b, steps)
        for cfg in CONFIGS:
            for k, v in cfg.items():
                ctx.set(k, v)
            got, fused, upd, mask, applied = _apply(ctx, dm, steps, b)
            what = "%s n=%d %s %s" % (kind, n, name, cfg)
            bits_equal(got, want, what)
            on = cfg["poly_fused"] == 1 and not FORCED and not scale
            expect_kernel(applied == 1, "%s: n_poly_apply moved by %d" % (what, applied))
            expect_kernel(fused == (nsteps if on else 0), "%s: %d fused launches" % (what, fused))
            expect_kernel(upd == (0 if on else nsteps), "%s: %d update launches" % (what, upd))
            if kind == "mask" and n >= 3 and cfg["spmv_dia"] == 1:
                expect_kernel(mask == (0 if scale else nsteps), "%s: n_dia_mask moved by %d" % (what, mask))
            if kind == "value" or cfg["spmv_dia"] == 0:
                expect_kernel(mask == 0, "%s: n_dia_mask moved by %d" % (what, mask))


@pytest.mark.parametrize("n", SIZES)
def test_oracle_bits_mask_form(switches, n):
    """A non-symmetric tridiagonal matrix with constant coefficients: the banded kernel's mask form."""
    A = pc.nonsym1d(n)
    dm = switches.csr(A)
    expect_kernel(n < 3 or dm.diagonals == 3, "nonsym1d(%d) has no banded form (%d diagonals)" % (n, dm.diagonals))
    _check_paths(switches, A, "mask", n)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_bits_value_form(switches, n):
    """The same with a varying diagonal: the banded kernel's value form."""
    _check_paths(switches, pc.nonsym1d(n, vary=True), "value", n)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_bits_csr_stream(switches, n):
    """A seeded random non-symmetric matrix of ~7 entries per row: the CSR-stream kernel, with and without its LDS window."""
    A = pc.random_nonsym(n, 7, seed=n)
    dm = switches.csr(A)
    expect_kernel(n < 64 or dm.diagonals == 0, "random_nonsym(%d) got a banded form" % n)
    _check_paths(switches, A, "stream", n)


def test_oracle_bits_five_diagonals_odd_rows(switches):
    """37 x 23 upwind convection-diffusion: five diagonals, an odd number of rows - the aligned row pairs and their tail; two
    columns, the second of which starts at an odd row offset of the block's leading dimension or not, as the block has it."""
    A = bc.convdiff(37, 23, 1.0, 0.3)
    n = A.shape[0]
    dm = switches.csr(A)
    expect_kernel(dm.diagonals == 5, "convdiff has %d diagonals" % dm.diagonals)
    b = _rhs(n, 2, seed=37)
    for name in ("lin5", "pairs2", "r-pair-r", "r-r-pair"):
        steps = pc.table(name)
        want = ref.poly_apply_ref(A, b, steps)
        for on in (1, 0):
            switches.set("poly_fused", on)
            got, fused, upd, _, applied = _apply(switches, dm, steps, b)
            bits_equal(got, want, "convdiff 37x23 %s fused=%d" % (name, on))
            k = 2 * steps.shape[0]
            expect_kernel((fused, upd) == ((k, 0) if on and not FORCED else (0, k)) and applied == 2,
                          "convdiff %s fused=%d: %d fused, %d update launches" % (name, on, fused, upd))


def test_row_longer_than_the_tile(switches):
    """A dense first row at n = 4099 takes the kernel's long-row branch (a tree sum): fused equals composed bit for bit, and
    the oracle at 1e-12."""
    n = 4099
    A = pc.random_nonsym(n, 7, seed=9).tolil()
    A[0, 1:] = 1e-3
    A[1:, 0] = -2e-3
    A[0, 0] = A[0, 0] + 5.0
    A = A.tocsr()
    A.sort_indices()
    dm = switches.csr(A)
    b = _rhs(n, 1, seed=5)
    for name in ("lin5", "r-pair-r"):
        steps = pc.table(name)
        switches.set("poly_fused", 1)
        got_f, fused, _, _, _ = _apply(switches, dm, steps, b)
        switches.set("poly_fused", 0)
        got_c, none, _, _, _ = _apply(switches, dm, steps, b)
        bits_equal(got_f, got_c, "long row, fused against composed")
        want = ref.poly_apply_ref(A, b, steps)
        assert np.linalg.norm(got_f - want) <= 1e-12 * np.linalg.norm(want)
        expect_kernel(fused == (0 if FORCED else steps.shape[0]) and none == 0, "long row: %d / %d fused launches" % (fused, none))


@pytest.mark.parametrize("kind,n", [("mask", 4099), ("stream", 2049), ("dense", 65)])
@pytest.mark.parametrize("fused", [1, 0])
def test_storage_contracts(switches, kind, n, fused):
    """Poisoned scratch and Y, both allocated unwritten: the same bits, x unchanged, nothing outside Y's columns written, the
    padding stays zero, two calls are bit-identical (ncols = 3)."""
    A = pc.nonsym1d(n) if kind == "mask" else pc.random_nonsym(n, 7, seed=1)
    ctx = switches
    ctx.set("poly_fused", fused)
    dm = ctx.dense(A.toarray()) if kind == "dense" else ctx.csr(A)
    b = _rhs(n, 3, seed=2)
    for name in ("r-pair-r", "pairs2", "lin1"):
        steps = pc.table(name)
        want = ref.poly_apply_ref(A, b, steps)
        with poisoned_allocations(ctx):
            X = ctx.upload(b)
            Y = ctx.alloc(n, 5, zero=False)
            S = ctx.alloc(n, 3, zero=False)
            out = []
            for _ in range(2):
                poison(Y)
                poison(S)
                ctx.poly_apply(dm, steps, X, 0, Y, 1, 3, S)
                out.append(Y.download(1, 3))
                assert not Y.padding_nonzero() and not S.padding_nonzero() and not X.padding_nonzero()
                assert np.all(np.isnan(Y.download(0, 1))) and np.all(np.isnan(Y.download(4, 1)))     # the neighbours are not written
            bits_equal(X.download(), b, "x is only read")
        if kind == "dense":
            assert np.linalg.norm(out[0] - want) <= 1e-13 * np.linalg.norm(want)      # (the dense kernel sums in another order)
        else:
            bits_equal(out[0], want, "poisoned blocks, %s %s fused=%d" % (kind, name, fused))
        bits_equal(out[0], out[1], "two calls")


def test_poly_update_alone(switches):
    """The composed steps on their own, [r, pair, r]: LIN first, QA, QB closing - the first step reads no y."""
    ctx = switches
    n = 2049
    A = pc.nonsym1d(n)
    steps = pc.table("r-pair-r")
    b = _rhs(n, 1, seed=6)
    X = ctx.upload(b)
    W = poison(ctx.alloc(n, 4, zero=False))            # prod 0 / 1, t, y
    dm = ctx.csr(A)
    u0 = ctx.get("n_poly_update")
    ctx.apply(dm, X, 0, W, 0, 1)
    ctx.poly_update(X, 0, None, 0, W, 3, W, 0, 0, steps[0, 1], first=True)
    ctx.apply(dm, W, 0, W, 2, 1)
    ctx.poly_update(W, 0, None, 0, W, 3, W, 2, 1, steps[1, 1], a2=steps[1, 2])
    ctx.apply(dm, W, 2, W, 1, 1)
    ctx.poly_update(W, 2, W, 0, W, 3, W, 1, 2, steps[2, 1], cl=steps[2, 4], close=True)
    bits_equal(W.download(3, 1), ref.poly_apply_ref(A, b, steps), "three composed steps")
    assert ctx.get("n_poly_update") - u0 == 3 and not W.padding_nonzero()
    bits_equal(X.download(), b, "x is only read")
    Y = poison(ctx.alloc(n, 1, zero=False))
    ctx.poly_update(X, 0, None, 0, Y, 0, None, 0, 3, 0.25, first=True)
    bits_equal(Y.download(), 0.25 * b, "SCALE")


def test_argument_errors(switches):
    from krypy_amd._hip import BackendError

    ctx = switches
    n = 130
    A = ctx.csr(pc.nonsym1d(n))
    Z = ctx.csr(pc.nonsym1d(n).astype(complex))
    st = pc.table("r-pair-r")
    X, Y, S = ctx.alloc(n, 4), ctx.alloc(n, 4), ctx.alloc(n, 3)
    Xc, Yc, Sc = (ctx.alloc(n, k, dtype=complex) for k in (2, 2, 3))
    ctx.poly_apply(A, st, X, 0, X, 2, 2, S)                   # one block, disjoint columns: fine
    bad = [
        ("overlap", lambda: ctx.poly_apply(A, st, X, 0, X, 0, 1, S)),
        ("overlap", lambda: ctx.poly_apply(A, st, X, 0, X, 1, 2, S)),
        ("scratch", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, ctx.alloc(n, 2))),
        ("scratch", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, X)),
        ("scratch", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, Y)),
        ("length|expected", lambda: ctx.poly_apply(A, st, ctx.alloc(n + 1, 1), 0, Y, 0, 1, S)),
        ("length|expected", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, ctx.alloc(n - 1, 3))),
        ("out of range", lambda: ctx.poly_apply(A, st, X, 3, Y, 0, 2, S)),
        ("real operators on real blocks only", lambda: ctx.poly_apply(A, st, Xc, 0, Yc, 0, 1, Sc)),
        ("real operators on real blocks only", lambda: ctx.poly_apply(Z, st, X, 0, Y, 0, 1, S)),
        ("real operators on real blocks only", lambda: ctx.poly_apply(Z, st, Xc, 0, Yc, 0, 1, Sc)),
        ("mixed", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, Sc)),
        ("diagonal", lambda: ctx.poly_apply(ctx.diag(np.ones(n)), st, X, 0, Y, 0, 1, S)),
        ("table", lambda: ctx.poly_apply(A, np.zeros(5), X, 0, Y, 0, 1, S)),
        ("at least 1", lambda: ctx.poly_apply(A, np.zeros((0, 5)), X, 0, Y, 0, 1, S)),
        ("kind 4", lambda: ctx.poly_apply(A, [[4, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("kind -1", lambda: ctx.poly_apply(A, [[-1, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("kind 0.5", lambda: ctx.poly_apply(A, [[0.5, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("closes on a QA", lambda: ctx.poly_apply(A, [[1, 1, 1, 1, 1]], X, 0, Y, 0, 1, S)),
        ("stand alone", lambda: ctx.poly_apply(A, [[3, 1, 0, 0, 0], [0, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("stand alone", lambda: ctx.poly_apply(A, [[0, 1, 0, 0, 0], [3, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("not preceded by QA", lambda: ctx.poly_apply(A, [[0, 1, 0, 0, 0], [2, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("not preceded by QA", lambda: ctx.poly_apply(A, [[2, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        # kh_poly_update
        ("different columns", lambda: ctx.poly_update(X, 0, None, 0, X, 0, S, 0, 0, 1.0, first=True)),
        ("different columns", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, X, 0, 0, 1.0)),
        ("different columns", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, Y, 0, 0, 1.0)),
        ("different columns", lambda: ctx.poly_update(X, 0, S, 0, Y, 0, S, 0, 2, 1.0)),
        ("different columns", lambda: ctx.poly_update(X, 0, Y, 0, Y, 0, S, 0, 2, 1.0)),
        ("expected", lambda: ctx.poly_update(X, 0, None, 0, ctx.alloc(n + 2, 1), 0, S, 0, 0, 1.0)),
        ("mixed", lambda: ctx.poly_update(X, 0, None, 0, Yc, 0, S, 0, 0, 1.0)),
        ("real operator on", lambda: ctx.poly_update(Xc, 0, None, 0, Yc, 0, Sc, 0, 0, 1.0)),
        ("kind 7", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, S, 0, 7, 1.0)),
        ("close on a QA", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, S, 0, 1, 1.0, close=True)),
        ("close on a SCALE", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, None, 0, 3, 1.0, close=True)),
        ("cannot be the first", lambda: ctx.poly_update(X, 0, X, 1, Y, 0, S, 0, 2, 1.0, first=True)),
        ("NULL", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, None, 0, 0, 1.0)),
        ("NULL", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, S, 0, 2, 1.0)),
    ]
    for pattern, call in bad:
        with pytest.raises(BackendError, match=pattern):
            call()


# ---- the shared cases on the device --------------------------------------------------------------------------------------------
def test_tables_refusals_and_order(hip):
    pc.case_tables()
    pc.case_refusals()
    pc.case_leja()
    pc.case_attributes()


def test_residual_polynomial_against_the_eigendecomposition(hip):
    for d in (2, 4, 8):
        pc.case_residual_polynomial(d)
    r = [pc.case_residual_polynomial(d, start=True) for d in (1, 2, 3, 4, 6, 8)]
    assert all(a > b for a, b in zip(r, r[1:]))


def test_invariant_subspace_and_warning(hip):
    pc.case_invariant_subspace()
    pc.case_unreliable_degree_warns()


def test_in_place_application_moves_x_out_of_the_way(hip):
    pc.case_in_place(hip)


@pytest.mark.parametrize("name", ["lin1", "lin5", "pairs2", "r-pair-r", "r-r-pair", "lin19"])
def test_generic_operator_path(hip, name):
    """A as a product of two operators: one ``A._apply_dev`` and one ``poly_update`` per step; the oracle's bits with the
    product formed the same way, and the matrix path's result within rounding."""
    f0 = hip.get("n_poly_fused")
    pc.case_generic(4099, name, lambda k: hip.get("n_" + k))
    expect_kernel(FORCED or hip.get("n_poly_fused") - f0 == (0 if name == "lin1" else pc.table(name).shape[0] * 2),
                  "generic path: the matrix twin's fused launches moved by %d" % (hip.get("n_poly_fused") - f0))


def test_matrix_path_equals_generic_path_bits(hip):
    """The same matrix as a ``MatrixLinearOperator`` (one library call) and wrapped in a composite ``A * 1.0`` (generic path:
    ``1.0 * s + 0.0 * s`` is ``s``): the same bits."""
    from krypy_amd import utils

    n = 4099
    A = pc.nonsym1d(n)
    b = _rhs(n, 2, seed=8)
    for name in ("lin5", "r-pair-r", "r-r-pair"):
        mat = utils.GmresPolynomialOperator(A, pc.ROOTS[name])
        gen = utils.GmresPolynomialOperator(utils.MatrixLinearOperator(A) * 1.0, pc.ROOTS[name])
        a0, u0 = hip.get("n_poly_apply"), hip.get("n_poly_update")
        ym = mat.dot(b)
        assert hip.get("n_poly_apply") - a0 == 2
        u1 = hip.get("n_poly_update")
        yg = gen.dot(b)
        assert hip.get("n_poly_apply") - a0 == 2 and hip.get("n_poly_update") - u1 == 2 * mat.steps.shape[0]
        bits_equal(ym, yg, "matrix path against generic path, %s" % name)
        bits_equal(ym, ref.poly_apply_ref(A, b, mat.steps), name)
        assert FORCED or u1 == u0


@pytest.mark.parametrize("name", sorted(pc.SYSTEMS))
def test_roots_from_the_device_arnoldi(hip, name):
    pc.case_roots(name)


@pytest.mark.parametrize("name", sorted(pc.SYSTEMS))
def test_gmres_takes_at_most_a_quarter_of_the_iterations(hip, name):
    """On the NumPy double: 80 -> 14, 83 -> 16, 94 -> 17 iterations."""
    pc.case_iteration_cap(name)


@pytest.mark.parametrize("solver,key", pc.TWINS)
def test_solvers_against_host_callable_twins(hip, solver, key):
    from krypy_amd import utils

    A, _ = pc.system("cd24")
    roots = pc.reference_roots("cd24")
    op = utils.GmresPolynomialOperator(A, roots)
    twin = pc.Twin(A, ref.steps_ref(roots))
    s0 = hip.get("n_poly_apply")
    res_d, x_d = pc.run_solver(solver, key, op)
    applied = hip.get("n_poly_apply") - s0
    res_t, x_t = pc.run_solver(solver, key, twin.op)
    bits_equal(res_d, res_t, "resnorms")
    bits_equal(x_d, x_t, "xk")
    assert applied == twin.calls and applied >= len(res_d) - 1
    assert hip.get("n_poly_apply") - s0 == applied          # the twin's run never touched the kernels
    assert res_d[-1] <= pc.TOL and len(res_d) - 1 < 60
