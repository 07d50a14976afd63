"""CPU tests of BiCGStab: the NumPy reference against itself (four summation orders), and the host layer
(``linsys.Bicgstab``, ``krypy_amd.bicgstab``) on a NumPy context whose ``bicgstab_*`` entries are that reference."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bicgstab_cases as bc
from tests.support import bicgstab_ref as ref


@pytest.fixture
def bicg_double():
    from krypy_amd import _hip
    from tests.support.bicgstab_numpy_context import BicgstabNumpyContext

    ctx = BicgstabNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_convdiff_is_the_definition():
    A = bc.convdiff(4, 3, 0.5, 0.25).toarray()
    assert A.shape == (12, 12)
    assert A[5, 5] == (2 + 0.5) + (2 + 0.25)
    assert A[5, 4] == -1.5 and A[5, 6] == -1.0 and A[5, 1] == -1.25 and A[5, 9] == -1.0
    assert A[4, 3] == 0.0 and A[3, 4] == 0.0                    # no coupling across the end of a grid row
    L = bc.convdiff(5, 4, 0, 0)
    assert abs(L - L.T).max() == 0.0


@pytest.mark.parametrize("name", sorted(bc.SYSTEMS))
def test_reference_orders_agree(name):
    """The four summation orders of the reference: the same residual norms to 2.5e-11 through iteration 10 (the issue
    measured 1.6e-14 at iteration 5 and at most 2.2e-11 at iteration 10; 1e-9, the bound of the solver tests, is 40 times
    that), iteration counts within the 15 % the solver tests allow, every run converged."""
    refs = bc.reference(name)
    A, b = bc.system(name)
    spread5, spread10 = bc.order_spread(name, 5), max(bc.order_spread(name, k) for k in range(1, 11))
    counts = sorted(r.iter for r in refs.values())
    print("%s: spread at 5 %.2e, through 10 %.2e, iterations %s" % (name, spread5, spread10, counts))
    assert spread10 <= 2.5e-11
    for r in refs.values():
        assert r.breakdown is None and r.resnorms[-1] <= bc.TOL
        assert bc.relres(A, r.x, b) <= 1e-7
    assert counts[-1] <= 1.15 * counts[0]


def test_step_ref_is_one_iteration_of_solve_ref():
    A, b = bc.system("cd24-rng")
    full = ref.solve_ref(A, b, 0.0, 3)
    st = dict(apply=A.dot, r=b.copy(), p=b.copy(), v=np.zeros(b.size), y=np.zeros(b.size))
    rt = b.copy()
    rho_prev = alpha = omega = 0.0
    rho = float(np.dot(rt, b))
    for k in range(3):
        _, rho_k, sigma, ss, theta, phi, rho_new, rr, _ = full.trace[k]
        assert rho_k == rho
        beta = (rho / rho_prev) * (alpha / omega) if k else 0.0
        out = ref.step_ref(st, dict(first=k == 0, beta=beta, omega_prev=omega, rho=rho, sigma=sigma, theta=theta, phi=phi))
        assert float(np.dot(out["s"], out["s"])) == ss and float(np.dot(out["r"], out["r"])) == rr
        assert float(np.dot(rt, out["r"])) == rho_new
        st.update(r=out["r"], p=out["p"], v=out["v"], y=out["y"])
        alpha, omega, rho_prev, rho = out["alpha"], out["omega"], rho, rho_new
    assert np.array_equal(st["y"], full.x)


# ---- the host layer on the double ---------------------------------------------------------------------------------------
def test_multiple_of_identity(bicg_double):
    bc.case_multiple_of_identity()


def test_swap_breakdown(bicg_double):
    bc.case_swap_breakdown()


@pytest.mark.parametrize("name", sorted(bc.SYSTEMS))
def test_whole_solve(bicg_double, name):
    sol = bc.case_whole_solve(name)
    # a plain matrix: every iteration is one bicgstab_step call, none of the pieces
    assert bicg_double.calls["bicgstab_step"] == sol.iter
    assert "bicgstab_half" not in bicg_double.calls and "apply" not in bicg_double.calls


def test_double_and_reference_are_the_same_bits(bicg_double):
    """numpy.dot in both: the solver on the double reproduces solve_ref's trace exactly"""
    A, b = bc.system("cd37x23-rng")
    sol = bc.solve(A, b)
    want = ref.solve_ref(A, b, bc.TOL, b.size)
    assert list(sol.bicgstab_trace) == want.trace[-len(sol.bicgstab_trace):]
    assert sol.iter == want.iter


def test_initial_guess(bicg_double):
    bc.case_initial_guess()


def test_shapes(bicg_double):
    bc.case_shapes()


def test_zero_rhs(bicg_double):
    bc.case_zero_rhs()
    assert not any(k.startswith("bicgstab") for k in bicg_double.calls)


def test_maxiter(bicg_double):
    bc.case_maxiter()


@pytest.mark.parametrize("side", ["Ml", "Mr"])
def test_generic_path(bicg_double, side):
    made = bc.case_generic(side, lambda: bicg_double.calls.get("bicgstab_step", 0))
    assert made == 0
    c = bicg_double.calls
    assert c["bicgstab_half"] == c["bicgstab_full"] == c["bicgstab_dir"] + 1


def test_host_callable_operator(bicg_double):
    """an operator that is a host callable goes the generic path and computes the same sequence as the fused one"""
    from krypy_amd import utils
    A, b = bc.system("cd24-ones")
    op = utils.LinearOperator(A.shape, float, dot=lambda X: A.dot(X))
    s_op, s_mat = bc.solve(op, b), bc.solve(A, b)
    assert s_op.resnorms == s_mat.resnorms and np.array_equal(s_op.xk, s_mat.xk)


def test_explicit_residual_and_errnorms(bicg_double):
    from krypy_amd import linsys
    A, b = bc.system("cd24-ones")
    x = np.linalg.solve(A.toarray(), b)
    sol = linsys.Bicgstab(linsys.LinearSystem(A, b, exact_solution=x), tol=bc.TOL, explicit_residual=True)
    assert sol.resnorms[-1] <= bc.TOL and len(sol.errnorms) == len(sol.resnorms)
    assert sol.errnorms[-1] <= 1e-6 * np.linalg.norm(x)


def test_refusals(bicg_double):
    bc.case_refusals()


def test_convenience(bicg_double):
    bc.case_convenience()


def test_double_refuses_what_the_library_refuses(bicg_double):
    from krypy_amd import _hip
    ctx = bicg_double
    B = ctx.alloc(6, 7)
    short = ctx.alloc(5, 1)
    A = ctx.csr(sp.identity(6, format="csr"))
    with pytest.raises(_hip.BackendError):
        ctx.bicgstab_dir(B, 0, B, 0, B, 1, 1.0, 1.0)
    with pytest.raises(_hip.BackendError):
        ctx.bicgstab_half(B, 0, B, 1, B, 2, B, 2, 1.0)
    with pytest.raises(_hip.BackendError):
        ctx.bicgstab_step(A, B, 0, B, 1, B, 2, B, 3, B, 4, B, 5, B, 5, True, 0.0, 0.0, 1.0)
    with pytest.raises(_hip.BackendError):
        ctx.bicgstab_step(A, B, 0, B, 1, B, 2, B, 3, B, 4, B, 5, short, 0, True, 0.0, 0.0, 1.0)
    with pytest.raises(_hip.BackendError):
        ctx.bicgstab_step(ctx.csr(sp.identity(6, format="csr").astype(complex)), B, 0, B, 1, B, 2, B, 3, B, 4, B, 5, B, 6,
                          True, 0.0, 0.0, 1.0)
