"""The BiCGStab cases that tests/test_bicgstab_host.py (on the NumPy double) and tests/test_gpu_bicgstab.py (on the device)
both run - TEST INFRASTRUCTURE ONLY.  Every function works on whatever context is installed."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bicgstab_ref as ref

TOL = 1e-8


def convdiff(nx, ny, cx, cy):
    """Five-point diffusion plus first-order upwind convection on an nx x ny grid, row-major:
    kron(I_ny, Tx) + kron(Ty, I_nx), Tx = tridiag(-(1 + cx), 2 + cx, -1), Ty likewise with cy.  CSR."""
    def tri(m, c):
        return sp.diags([np.full(m - 1, -(1.0 + c)), np.full(m, 2.0 + c), np.full(m - 1, -1.0)], [-1, 0, 1])
    return sp.csr_matrix(sp.kron(sp.identity(ny), tri(nx, cx)) + sp.kron(tri(ny, cy), sp.identity(nx)))


def scaled_system():
    """convdiff(24, 24, 0.5, 0.25) with a position-dependent diagonal added, so that a diagonal scaling matters"""
    A = convdiff(24, 24, 0.5, 0.25)
    n = A.shape[0]
    return sp.csr_matrix(A + sp.diags(1.0 + (np.arange(n) % 7))), np.ones(n)


def rhs(n, kind):
    return np.ones(n) if kind == "ones" else np.random.default_rng(1).standard_normal(n)


SYSTEMS = {
    "cd24-ones": (lambda: convdiff(24, 24, 0.5, 0.25), "ones"),
    "cd24-rng": (lambda: convdiff(24, 24, 0.5, 0.25), "rng"),
    "cd37x23-ones": (lambda: convdiff(37, 23, 1.0, 0.3), "ones"),
    "cd37x23-rng": (lambda: convdiff(37, 23, 1.0, 0.3), "rng"),
    "lap24-rng": (lambda: convdiff(24, 24, 0.0, 0.0), "rng"),
}


@functools.lru_cache(maxsize=None)
def system(name):
    make, kind = SYSTEMS[name]
    A = make()
    return A, rhs(A.shape[0], kind)


@functools.lru_cache(maxsize=None)
def reference(name):
    """solve_ref on a named system in the four summation orders (computed once per process, never modified)"""
    A, b = system(name)
    return {o: ref.solve_ref(A, b, TOL, A.shape[0], dot=d) for o, d in ref.DOTS.items()}


def order_spread(name, k):
    """largest relative difference of resnorms[k] between the four summation orders of the reference"""
    v = np.array([r.resnorms[k] for r in reference(name).values()])
    return float((v.max() - v.min()) / v.min())


def relres(A, x, b):
    x = np.asarray(x).reshape(-1)
    return np.linalg.norm(b.reshape(-1) - A.dot(x)) / np.linalg.norm(b)


def solve(A, b, **kw):
    from krypy_amd import linsys
    lskw = {k: kw.pop(k) for k in ("Ml", "Mr") if k in kw}
    kw.setdefault("tol", TOL)
    return linsys.Bicgstab(linsys.LinearSystem(A, b, **lskw), **kw)


# ---- clamp and breakdown ------------------------------------------------------------------------------------------------
def case_multiple_of_identity():
    """A = 2 I: alpha = 1/2 exactly, s = 0, t = 0, omega = 0/0 clamped to 0, r = 0: one iteration, x = b / 2"""
    from krypy_amd import _hip
    b = np.array([1.0, -2.0, 3.0, 0.5, 4.0])
    sol = solve(sp.csr_matrix(2.0 * sp.identity(5)), b)
    assert sol.iter == 1
    assert np.array_equal(sol.xk.reshape(-1), b / 2)
    assert len(sol.bicgstab_trace) == 1 and sol.bicgstab_trace[0][-1] & _hip.BICG_OMEGA_CLAMPED
    assert sol.resnorms[-1] == 0.0


def case_swap_breakdown():
    """A = [[0, 1], [1, 0]], b = e_1: <rt, v> = 0 in the first iteration"""
    from krypy_amd import utils
    with pytest.raises(utils.ConvergenceError, match="BiCGStab breakdown in iteration 0") as ei:
        solve(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), np.array([1.0, 0.0]))
    assert "alpha clamped" in str(ei.value)
    sol = ei.value.solver
    assert np.all(np.isfinite(sol.xk)) and sol.xk.shape == (2, 1)
    assert len(sol.bicgstab_trace) == 1


# ---- whole solves -------------------------------------------------------------------------------------------------------
def case_whole_solve(name):
    A, b = system(name)
    refs = reference(name)
    sol = solve(A, b)
    assert sol.resnorms[-1] <= TOL
    assert relres(A, sol.xk, b) <= TOL * (1 + 1e-6)
    want = np.array(refs["numpy"].resnorms[1:9])
    got = np.array(sol.resnorms[1:9])
    print("%s: iter %d (reference %s), resnorms[1:9] max rel diff %.3e" % (
        name, sol.iter, sorted(r.iter for r in refs.values()), np.max(np.abs(got - want) / want)))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
    assert sol.iter <= math.ceil(1.15 * max(r.iter for r in refs.values()))
    return sol


def case_initial_guess():
    A, b = system("cd24-ones")
    x0 = np.random.default_rng(7).standard_normal(b.size)
    s0, s1 = solve(A, b), solve(A, b, x0=x0)
    assert s1.resnorms[-1] <= TOL
    assert np.linalg.norm(s1.xk - s0.xk) <= 1e-6 * np.linalg.norm(s0.xk)


def case_shapes():
    A, b = system("cd24-ones")
    flat, col = solve(A, b), solve(A, b.reshape(-1, 1))
    assert flat.linear_system.flat_vecs and not col.linear_system.flat_vecs      # (xk is (N, 1) either way, as in Cg / Gmres)
    assert flat.xk.shape == (b.size, 1) and col.xk.shape == (b.size, 1)
    assert flat.resnorms == col.resnorms


def case_zero_rhs():
    A, b = system("cd24-ones")
    sol = solve(A, np.zeros(b.size))
    assert sol.resnorms == [0.0] and sol.iter == 0
    assert not np.any(sol.xk)


def case_maxiter():
    from krypy_amd import utils
    A, b = system("cd24-ones")
    with pytest.raises(utils.ConvergenceError) as ei:
        solve(A, b, maxiter=3)
    assert ei.value.solver.iter == 3
    assert len(ei.value.solver.resnorms) == 4


def case_generic(side, step_calls):
    """Ml or Mr = the inverse diagonal: a composite operator, so the generic path; ``step_calls()``: how many
    bicgstab_step calls the context has seen."""
    A, b = scaled_system()
    D = sp.diags(1.0 / A.diagonal())
    kw = {side: D}
    before = step_calls()
    sol = solve(A, b, **kw)
    made = step_calls() - before
    assert sol.resnorms[-1] <= TOL
    want = ref.solve_ref(A, b, TOL, b.size, **kw)
    np.testing.assert_allclose(sol.resnorms[1:9], want.resnorms[1:9], rtol=1e-9, atol=0)
    # residual of the preconditioned system: ||Ml (b - A x)|| / ||Ml b||
    Ml = D if side == "Ml" else sp.identity(b.size)
    x = sol.xk.reshape(-1)
    assert np.linalg.norm(Ml.dot(b - A.dot(x))) / np.linalg.norm(Ml.dot(b)) <= TOL * (1 + 1e-6)
    return made


def case_refusals():
    from krypy_amd import linsys, utils
    A, b = system("cd24-ones")
    n = b.size
    Id = sp.identity(n, format="csr")
    with pytest.raises(utils.ArgumentError, match="Ml"):
        linsys.Bicgstab(linsys.LinearSystem(A, b, M=sp.diags(np.full(n, 2.0))))
    with pytest.raises(utils.ArgumentError, match="Ml"):
        linsys.Bicgstab(linsys.LinearSystem(A, b, Minv=sp.diags(np.full(n, 2.0))))
    with pytest.raises(utils.ArgumentError, match="inner product"):
        linsys.Bicgstab(linsys.LinearSystem(A, b, ip_B=sp.diags(np.full(n, 2.0))))
    linsys.Bicgstab(linsys.LinearSystem(A, b, ip_B=None, M=None), tol=TOL)
    with pytest.raises(utils.ArgumentError, match="store_arnoldi"):
        linsys.Bicgstab(linsys.LinearSystem(A, b), store_arnoldi=True)
    with pytest.raises(NotImplementedError):
        linsys.Bicgstab(linsys.LinearSystem(A.astype(complex), b))
    with pytest.raises(NotImplementedError):
        linsys.Bicgstab(linsys.LinearSystem(A, b.astype(complex)))
    with pytest.raises(NotImplementedError):
        linsys.Bicgstab(linsys.LinearSystem(A, b), x0=np.zeros(n, dtype=complex))
    with pytest.raises(NotImplementedError):
        linsys.Bicgstab(linsys.LinearSystem(A, b, Ml=Id.astype(complex) * 2))
    with pytest.raises(NotImplementedError):
        linsys.Bicgstab(linsys.LinearSystem(A, b, Mr=Id.astype(complex) * 2))
    with pytest.raises(utils.ArgumentError):
        linsys.Bicgstab("not a linear system")


def case_convenience():
    import krypy_amd
    from krypy_amd import linsys
    A, b = system("cd24-ones")
    for shape in ((b.size,), (b.size, 1)):
        x, sol = krypy_amd.bicgstab(A, b.reshape(shape), tol=TOL)
        assert isinstance(sol, linsys.Bicgstab)
        assert x.shape == shape and relres(A, x, b) <= TOL * (1 + 1e-6)
    # "not converged" for the wrappers is resnorms[-1] >= tol: A = 2 I ends with a residual of exactly 0, which is not
    # below a tolerance of 0 (a solve that runs out of iterations raises instead, as in the other wrappers)
    x, sol = krypy_amd.bicgstab(sp.csr_matrix(2.0 * sp.identity(5)), np.arange(1.0, 6.0), tol=0.0)
    assert x is None and sol.resnorms[-1] == 0.0 and sol.iter == 1
    assert "krypy BiCGStab object" in repr(krypy_amd.bicgstab(A, b, tol=TOL)[1])
    assert linsys.Bicgstab.operations(3) == {"A": 7, "M": 2, "Ml": 8, "Mr": 7, "ip_B": 17, "axpy": 19}
