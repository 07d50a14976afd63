"""CPU tests of the Chebyshev polynomial preconditioner: the coefficients, the oracle's operator (symmetric, positive definite),
and the host layer (``utils.ChebyshevOperator``, ``utils.chebyshev_operator``) on a NumPy context whose ``cheb_update`` /
``cheb_apply`` are the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import cheb_cases as cc
from tests.support.cheb_ref import cheb_apply_ref, cheb_coefficients


@pytest.fixture
def cheb_double():
    from krypy_amd import _hip
    from tests.support.cheb_numpy_context import ChebNumpyContext

    ctx = ChebNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# ---- coefficients --------------------------------------------------------------------------------------------------
def test_coefficients_degree_3_by_hand(cheb_double):
    """lmin = 1, lmax = 3: theta = 2, delta = 1, sigma = 2, rho_0 = 1/2, rho_1 = 1/(4 - 1/2) = 2/7, rho_2 = 1/(4 - 2/7) = 7/26:
    (a, b) = (0, 1/2), (1/7, 4/7), (1/13, 7/13)."""
    from krypy_amd import utils

    want = np.array([[0.0, 0.5], [1.0 / 7.0, 4.0 / 7.0], [1.0 / 13.0, 7.0 / 13.0]])
    got = utils.ChebyshevOperator(cc.lap1d(5), 3.0, lmin=1.0, degree=3).coefficients
    assert got.shape == (3, 2) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=4e-16, atol=0)
    assert np.array_equal(got, cheb_coefficients(1.0, 3.0, 3))        # the package and the oracle: the same bits
    op = utils.ChebyshevOperator(cc.lap1d(5), 6.0, degree=2)
    assert op.lmin == 6.0 / 30.0 and op.lmax == 6.0 and op.degree == 2


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("degree", [1, 2, 4, 7])
def test_assembled_operator_is_spd(cheb_double, degree, scaled):
    """M applied to the identity on the 7 x 5 grid: symmetric to 1e-15 relative, positive definite; with a scaling s the
    operator is p(D^-1 A) D^-1, symmetric as well."""
    from krypy_amd import utils

    A = cc.lap2d(7, 5)
    n = A.shape[0]
    s = np.random.default_rng(5).uniform(0.5, 2.0, n) if scaled else None
    lmax = 8.0 / (0.5 if scaled else 1.0)
    op = utils.ChebyshevOperator(A, lmax, degree=degree, scale=s)
    M = op.dot(np.eye(n))
    assert np.linalg.norm(M - M.T) <= 1e-15 * np.linalg.norm(M)
    assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0
    assert np.array_equal(M, cheb_apply_ref(A, np.eye(n), op.coefficients, None if s is None else 1.0 / s))
    assert op.adj is op
    assert np.array_equal(op.dot_adj(np.eye(n)), M)


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_argument_errors(cheb_double):
    from krypy_amd import utils

    A = cc.lap2d(4, 3)
    E = utils.ArgumentError
    with pytest.raises(E, match="square"):
        utils.ChebyshevOperator(sp.csr_matrix(np.ones((3, 4))), 2.0)
    with pytest.raises(E, match="degree"):
        utils.ChebyshevOperator(A, 8.0, degree=0)
    for lmax, lmin in ((8.0, 8.0), (8.0, 0.0), (8.0, -1.0), (-1.0, None), (1.0, 2.0), (np.inf, 1.0)):
        with pytest.raises(E, match="0 < lmin < lmax"):
            utils.ChebyshevOperator(A, lmax, lmin=lmin)
    bad = np.ones(12)
    bad[3] = 0.0
    with pytest.raises(E, match="positive"):
        utils.ChebyshevOperator(A, 8.0, scale=bad)
    bad[3] = -2.0
    with pytest.raises(E, match="positive"):
        utils.ChebyshevOperator(A, 8.0, scale=bad)
    with pytest.raises(E, match="complex"):
        utils.ChebyshevOperator(A, 8.0, scale=np.ones(12) + 1j)
    with pytest.raises(E, match="shape"):
        utils.ChebyshevOperator(A, 8.0, scale=np.ones(11))
    with pytest.raises(E, match="shape"):
        utils.ChebyshevOperator(A, 8.0, scale=np.ones((12, 1)))
    with pytest.raises(E, match="jacobi"):
        utils.ChebyshevOperator(utils.MatrixLinearOperator(A) * utils.MatrixLinearOperator(A), 64.0, scale="jacobi")
    with pytest.raises(E, match="scale"):
        utils.ChebyshevOperator(A, 8.0, scale="ssor")


def test_backend_argument_errors(cheb_double):
    """The double refuses what the library refuses: x and y the same column, a scratch that is too small or overlaps."""
    from krypy_amd._hip import BackendError

    ctx = cheb_double
    A = ctx.csr(cc.lap1d(6))
    coef = cheb_coefficients(0.1, 4.0, 3)
    X, Y, S = ctx.alloc(6, 2), ctx.alloc(6, 2), ctx.alloc(6, 3)
    with pytest.raises(BackendError, match="overlap"):
        ctx.cheb_apply(A, None, coef, X, 0, X, 0, 1, S)
    with pytest.raises(BackendError, match="scratch"):
        ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, ctx.alloc(6, 2))
    with pytest.raises(BackendError, match="scratch"):
        ctx.cheb_apply(A, None, coef, X, 0, Y, 0, 1, X)
    with pytest.raises(BackendError, match="Dinv"):
        ctx.cheb_apply(A, ctx.diag(np.ones(5)), coef, X, 0, Y, 0, 1, S)
    with pytest.raises(BackendError, match="operator on"):
        ctx.cheb_apply(A, None, coef, ctx.alloc(6, 1, dtype=complex), 0, ctx.alloc(6, 1, dtype=complex), 0, 1,
                       ctx.alloc(6, 3, dtype=complex))


# ---- dtypes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_narrow_input_is_promoted_to_fp64(cheb_double, dtype):
    from krypy_amd import utils

    A = cc.lap2d(5, 4).astype(dtype)
    op = utils.ChebyshevOperator(A, 8.0, degree=3, scale="jacobi")
    assert op.dtype == np.float64
    b = np.arange(1.0, 21.0).reshape(-1, 1)
    y = op.dot(b)
    assert y.dtype == np.float64
    assert np.array_equal(y, cheb_apply_ref(A.astype(np.float64), b, op.coefficients, 1.0 / A.diagonal().astype(float)))


@pytest.mark.parametrize("scaled", [False, True])
def test_real_operator_on_complex_vectors(cheb_double, scaled):
    from krypy_amd import utils

    A = cc.lap2d(5, 4)
    s = np.linspace(1.0, 2.0, 20) if scaled else None
    op = utils.ChebyshevOperator(A, 8.0, degree=4, scale=s)
    rng = np.random.default_rng(1)
    b = rng.standard_normal((20, 2)) + 1j * rng.standard_normal((20, 2))
    y = op.dot(b)
    assert y.dtype == np.complex128
    dinv = None if s is None else 1.0 / s
    want = cheb_apply_ref(A, b.real, op.coefficients, dinv) + 1j * cheb_apply_ref(A, b.imag, op.coefficients, dinv)
    assert _rel(y, want) < 1e-14


def test_in_place_application_moves_r_out_of_the_way(cheb_double):
    from krypy_amd import utils

    A = cc.lap2d(5, 4)
    op = utils.ChebyshevOperator(A, 8.0, degree=3)
    b = np.random.default_rng(2).standard_normal((20, 2))
    X = cheb_double.upload(b)
    op._apply_dev(X, 0, X, 0, 2)
    assert np.array_equal(X.download(), cheb_apply_ref(A, b, op.coefficients))


# ---- the generic-operator path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("degree", [1, 2, 5])
def test_generic_operator_path_equals_matrix_path(cheb_double, degree, scaled):
    """A given as a product of two operators (B * B with B the 1-D Laplacian plus identity: A = B^2) goes through
    ``A._apply_dev`` + ``cheb_update``; the same A as one matrix through ``cheb_apply``."""
    from krypy_amd import utils

    B = (cc.lap1d(23) + sp.identity(23)).tocsr()
    A = (B @ B).tocsr()
    s = np.linspace(1.0, 3.0, 23) if scaled else None
    gen = utils.ChebyshevOperator(utils.MatrixLinearOperator(B) * utils.MatrixLinearOperator(B), 25.0, degree=degree, scale=s)
    mat = utils.ChebyshevOperator(A, 25.0, degree=degree, scale=s)
    b = np.random.default_rng(4).standard_normal((23, 3))
    before = dict(cheb_double.calls)
    yg = gen.dot(b)
    assert cheb_double.calls.get("cheb_update", 0) - before.get("cheb_update", 0) == 3 * degree
    assert cheb_double.calls.get("cheb_apply", 0) == before.get("cheb_apply", 0)
    ym = mat.dot(b)
    assert cheb_double.calls.get("cheb_apply", 0) - before.get("cheb_apply", 0) == 1
    assert _rel(yg, ym) < 1e-14           # (B (B z) and (B B) z round differently)
    # with the product formed the oracle's way the generic path has the oracle's bits
    class _BB(object):
        dtype = np.dtype(float)

        @staticmethod
        def dot(z):
            return B.dot(B.dot(z))
    assert np.array_equal(yg, cheb_apply_ref(_BB, b, gen.coefficients, None if s is None else 1.0 / s))


# ---- solvers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["Cg", "Minres", "Gmres"])
def test_solvers_agree_with_the_oracle_as_a_callable(cheb_double, solver):
    from krypy_amd import linsys, utils

    A = cc.lap2d(9, 7)
    n = A.shape[0]
    b = np.random.default_rng(11).standard_normal((n, 1))
    op = utils.ChebyshevOperator(A, 8.0, degree=4)
    twin = utils.LinearOperator((n, n), float, dot=lambda X: cheb_apply_ref(A, X, op.coefficients))
    out = []
    for M in (op, twin):
        sol = getattr(linsys, solver)(linsys.LinearSystem(A, b, M=M, self_adjoint=True, positive_definite=True), tol=1e-10)
        out.append(sol)
    r0, r1 = np.array(out[0].resnorms), np.array(out[1].resnorms)
    assert r0.shape == r1.shape and len(r0) < 40
    assert np.max(np.abs(r0 - r1) / r1[0]) < 1e-12
    assert _rel(out[0].xk, out[1].xk) < 1e-12


# ---- the estimate of lmax -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
def test_lmax_estimate_brackets_the_largest_eigenvalue(cheb_double, scaled):
    from krypy_amd import utils

    A = cc.lap2d(37, 23)
    if scaled:
        s = np.random.default_rng(8).uniform(0.5, 2.0, A.shape[0])
        A = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
        d = A.diagonal()
        lam = np.linalg.eigvalsh((A.toarray() / np.sqrt(d)[:, None]) / np.sqrt(d)[None, :])[-1]
    else:
        lam = np.linalg.eigvalsh(A.toarray())[-1]
    op = utils.chebyshev_operator(A, scale="jacobi" if scaled else None)
    assert op.lmax_estimate == op.lmax and op.degree == 4 and op.lmin == op.lmax / 30.0
    assert lam <= op.lmax <= 1.1 * lam, (lam, op.lmax, op.lmax / lam)
    if scaled:
        assert np.array_equal(op.dinv, 1.0 / A.diagonal())
