"""CPU tests of the GMRES polynomial preconditioner: the roots, their order, the table of steps, and the host layer
(``polyprecond.GmresPolynomialOperator``, ``gmres_polynomial_operator``) on a NumPy context whose ``poly_update`` /
``poly_apply`` are the oracle (tests/support/poly_ref.py).  The cases are those of tests/test_gpu_poly.py."""
import numpy as np
import pytest

from tests.support import poly_cases as pc
from tests.support import poly_ref as ref


@pytest.fixture
def poly_double():
    from krypy_amd import _hip
    from tests.support.poly_numpy_context import PolyNumpyContext

    ctx = PolyNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


def test_tables_by_hand(poly_double):
    pc.case_tables()


def test_refusals(poly_double):
    pc.case_refusals()


def test_leja_order(poly_double):
    pc.case_leja()


def test_attributes_and_entry_points(poly_double):
    pc.case_attributes()


def test_residual_polynomial_against_the_eigendecomposition(poly_double):
    """... and with the start vector of the Arnoldi steps as ``w`` it falls with the degree (the GMRES residual)."""
    for d in (2, 4, 8):
        pc.case_residual_polynomial(d)
    r = [pc.case_residual_polynomial(d, start=True) for d in (1, 2, 3, 4, 6, 8)]
    assert all(a > b for a, b in zip(r, r[1:]))


def test_the_recorded_spreads_hold():
    """The two tolerances of poly_cases are 100 x what the oracle's four summation orders spread over; measured again here,
    with a factor 2 for another BLAS."""
    assert max(pc.order_spread_residual(d) for d in (4, 8)) <= pc.RTOL_RESIDUAL / 50
    assert max(pc.order_spread_roots(name) for name in pc.SYSTEMS) <= pc.RTOL_ROOTS / 50


def test_invariant_subspace(poly_double):
    pc.case_invariant_subspace()


def test_unreliable_degree_warns(poly_double):
    pc.case_unreliable_degree_warns()


def test_in_place_application_moves_x_out_of_the_way(poly_double):
    pc.case_in_place(poly_double)


@pytest.mark.parametrize("name", sorted(pc.ROOTS))
def test_update_steps_equal_the_whole_application(poly_double, name):
    """The double's ``poly_update``, driven step by step by the generic-operator path, gives the bits of ``poly_apply_ref``."""
    pc.case_generic(23, name, lambda k: poly_double.calls.get(k, 0))


def test_backend_argument_errors(poly_double):
    """The double refuses what the library refuses."""
    from krypy_amd._hip import BackendError

    ctx = poly_double
    A = ctx.csr(pc.nonsym1d(6))
    st = pc.table("r-pair-r")
    X, Y, S = ctx.alloc(6, 2), ctx.alloc(6, 2), ctx.alloc(6, 3)
    bad = [
        ("overlap", lambda: ctx.poly_apply(A, st, X, 0, X, 0, 1, S)),
        ("scratch", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, ctx.alloc(6, 2))),
        ("scratch", lambda: ctx.poly_apply(A, st, X, 0, Y, 0, 1, X)),
        ("real operators on real blocks only", lambda: ctx.poly_apply(ctx.csr(pc.nonsym1d(6).astype(complex)), st, X, 0, Y, 0, 1, S)),
        ("diagonal", lambda: ctx.poly_apply(ctx.diag(np.ones(6)), st, X, 0, Y, 0, 1, S)),
        ("table", lambda: ctx.poly_apply(A, np.zeros(5), X, 0, Y, 0, 1, S)),
        ("kind", lambda: ctx.poly_apply(A, [[4, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("closes on a QA", lambda: ctx.poly_apply(A, [[1, 1, 1, 1, 1]], X, 0, Y, 0, 1, S)),
        ("stand alone", lambda: ctx.poly_apply(A, [[3, 1, 0, 0, 0], [0, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("not preceded by QA", lambda: ctx.poly_apply(A, [[0, 1, 0, 0, 0], [2, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("not preceded by QA", lambda: ctx.poly_apply(A, [[2, 1, 0, 0, 0]], X, 0, Y, 0, 1, S)),
        ("different columns", lambda: ctx.poly_update(X, 0, None, 0, X, 0, S, 0, 0, 1.0, first=True)),
        ("close on a QA", lambda: ctx.poly_update(X, 0, None, 0, Y, 0, S, 0, 1, 1.0, close=True)),
    ]
    for pattern, call in bad:
        with pytest.raises(BackendError, match=pattern):
            call()


@pytest.mark.parametrize("name", sorted(pc.SYSTEMS))
def test_roots_against_the_oracle(poly_double, name):
    pc.case_roots(name)


@pytest.mark.parametrize("name", sorted(pc.SYSTEMS))
def test_gmres_takes_at_most_a_quarter_of_the_iterations(poly_double, name):
    pc.case_iteration_cap(name)


@pytest.mark.parametrize("solver,key", pc.TWINS)
def test_solvers_agree_with_the_oracle_as_a_callable(poly_double, solver, key):
    from krypy_amd import utils

    A, _ = pc.system("cd24")
    op = utils.GmresPolynomialOperator(A, pc.reference_roots("cd24"))
    twin = pc.Twin(A, ref.steps_ref(pc.reference_roots("cd24")))
    r0, x0 = pc.run_solver(solver, key, op)
    r1, x1 = pc.run_solver(solver, key, twin.op)
    assert r0.shape == r1.shape and r0[-1] <= pc.TOL and twin.calls >= len(r1) - 1
    assert np.array_equal(r0, r1) and np.array_equal(x0, x1)
