"""The cases of the GMRES polynomial preconditioner that tests/test_poly_host.py (on the NumPy double) and tests/test_gpu_poly.py
(on the device) both run - TEST INFRASTRUCTURE ONLY.  Every function works on whatever context is installed."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bicgstab_cases as bc
from tests.support import idrs_cases as ic
from tests.support import poly_ref as ref
from tests.support.bicgstab_ref import DOTS

TOL = 1e-8
# |w - A p(A) w| / |w| against |pi(A) w| / |w| from the dense eigendecomposition, on the 24-row convdiff(6, 4, .5, .25) with the
# roots of poly_ref at degree 4 and 8.  Measured on the CPU between the four summation orders of bicgstab_ref.DOTS (the
# inner product of the Arnoldi steps that produce the roots): the left side moves by 6.5e-15 (degree 4) and 1.2e-14 (degree 8)
# relative; the two sides differ by at most 7.9e-15 there.  100 x the larger spread:
RTOL_RESIDUAL = 1.2e-12
# the roots at degree 8 on the three systems of SYSTEMS, sorted, relative to the largest modulus: between the four orders at most
# 2.9e-15 (cd24), 4.9e-15 (cd37x23), 2.6e-15 (central32).  100 x the largest; the device's order is a fifth one.
RTOL_ROOTS = 4.9e-13

SYSTEMS = {
    "cd24": lambda: bc.convdiff(24, 24, 0.5, 0.25),
    "cd37x23": lambda: bc.convdiff(37, 23, 1.0, 0.3),
    "central32": lambda: ic.central(32, 32, 4.0, 2.0),
}

# explicit synthetic roots (ordered: a pair's members adjacent), by name
ROOTS = {
    "lin1": [2.0],
    "lin2": [2.0, 3.5],
    "lin5": [4.5, 0.75, 2.5, 3.5, 1.5],
    "pair": [2.0 + 1.0j, 2.0 - 1.0j],
    "pairs2": [3.0 + 0.5j, 3.0 - 0.5j, 1.25 + 2.0j, 1.25 - 2.0j],
    "r-pair-r": [4.0, 2.0 + 1.5j, 2.0 - 1.5j, 1.0],             # a closing real root after a QB
    "r-r-pair": [4.0, 1.0, 2.5 + 0.75j, 2.5 - 0.75j],           # a closing pair
    "lin19": [0.5 + 0.25 * ((7 * i) % 19) for i in range(19)],  # 18 steps: crosses the 16-record chunk
}


@functools.lru_cache(maxsize=None)
def system(name):
    A = SYSTEMS[name]()
    return A, np.ones(A.shape[0])


def nonsym1d(n, vary=False):
    """A NON-symmetric tridiagonal matrix, tridiag(-1.5, 2.5, -1); ``vary``: a diagonal 2.5 + i / n (no constant coefficients:
    the value form)."""
    d = 2.5 + (np.arange(n) / float(n) if vary else np.zeros(n))
    if n == 1:
        return sp.csr_matrix(np.array([[d[0]]]))
    A = sp.diags([np.full(n - 1, -1.5), d, -np.ones(n - 1)], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return A


def random_nonsym(n, per_row=7, seed=0):
    """A seeded random NON-symmetric, strictly diagonally dominant matrix with about ``per_row`` entries per row at random places
    (no banded form: the CSR-stream kernel)."""
    rng = np.random.default_rng(seed)
    k = max(per_row - 1, 1)
    rows = np.repeat(np.arange(n), k)
    cols = rng.integers(0, n, size=n * k)
    vals = rng.uniform(-1.0, 1.0, size=n * k)
    keep = rows != cols
    B = sp.coo_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    diag = np.asarray(abs(B).sum(axis=1)).ravel() + 1.0 + rng.uniform(0.0, 1.0, size=n)
    A = (B + sp.diags(diag)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def order_spread_roots(name, degree=8):
    """largest difference of the sorted roots between the four summation orders of the oracle's Arnoldi steps, relative to the
    largest modulus (what RTOL_ROOTS is 100 x of)"""
    A, _ = system(name)
    rs = [np.sort_complex(ref.roots_ref(A, degree, dot=d)) for d in DOTS.values()]
    return float(max(np.max(np.abs(r - rs[0])) for r in rs) / np.max(np.abs(rs[0])))


def order_spread_residual(degree):
    """relative spread of ``|w - A p(A) w| / |w|`` on the 24-row matrix between the four summation orders (what RTOL_RESIDUAL
    is 100 x of)"""
    A = bc.convdiff(6, 4, 0.5, 0.25)
    w = np.random.default_rng(3).standard_normal(24)
    v = []
    for d in DOTS.values():
        y = ref.poly_apply_ref(A, w, ref.steps_ref(ref.roots_ref(A, degree, dot=d)))
        v.append(np.linalg.norm(w - A.dot(y)) / np.linalg.norm(w))
    return float((max(v) - min(v)) / min(v))


def table(name):
    return ref.steps_ref(ROOTS[name])


def relres(A, x, b):
    x = np.asarray(x).reshape(-1)
    return np.linalg.norm(b.reshape(-1) - A.dot(x)) / np.linalg.norm(b)


# ---- the table --------------------------------------------------------------------------------------------------------------
def case_tables():
    """Hand-written root sets against the walk written out by hand."""
    from krypy_amd import polyprecond as pp

    r, q = 4.0, 0.5
    a, b = 2.0, 1.5
    c = 1 / ((a * a) + (b * b))
    pair = [complex(a, b), complex(a, -b)]
    want = {
        "one real root": ([r], [[3, 1 / r, 0, 0, 0]]),
        "[r, r]": ([r, r], [[0, 1 / r, 0, 1, 1 / r]]),
        "one pair": (pair, [[1, c, 2 * a, 0, 0]]),
        "[pair, r]": (pair + [r], [[1, c, 2 * a, 0, 0], [2, c, 0, 1, 1 / r]]),
        "[r, pair]": ([r] + pair, [[0, 1 / r, 0, 0, 0], [1, c, 2 * a, 0, 0]]),
        "[r, pair, r, r]": ([r] + pair + [q, r], [[0, 1 / r, 0, 0, 0], [1, c, 2 * a, 0, 0], [2, c, 0, 0, 0],
                                                  [0, 1 / q, 0, 1, 1 / r]]),
        "conjugate first": (pair[::-1], [[1, c, 2 * a, 0, 0]]),
    }
    for what, (roots, rows) in want.items():
        got = pp.gmres_polynomial_steps(roots)
        assert got.dtype == np.float64 and got.shape == (len(rows), 5), what
        assert np.array_equal(got, np.array(rows, dtype=float)), what
        assert np.array_equal(got, ref.steps_ref(roots)), what
        assert len(roots) == 1 or got.shape[0] == len(roots) - 1, what
    for name, roots in ROOTS.items():
        got = pp.gmres_polynomial_steps(roots)
        assert np.array_equal(got, ref.steps_ref(roots)), name
        assert got.shape[0] == max(len(roots) - 1, 1), name


def case_refusals():
    from krypy_amd import polyprecond as pp
    from krypy_amd import utils

    E = utils.ArgumentError
    for roots, pattern in (([1.0 + 1.0j], "conjugation"), ([1.0 + 1.0j, 2.0, 1.0 - 1.0j], "conjugation"),
                           ([1.0 + 1.0j, 1.0 - 2.0j], "conjugation"), ([2.0, 0.0], "zero"), ([0.0j], "zero"),
                           ([1.0, np.inf], "finite"), ([np.nan], "finite"), ([], "at least one")):
        with pytest.raises(E, match=pattern):
            pp.gmres_polynomial_steps(roots)
    A = bc.convdiff(5, 4, 0.5, 0.25)
    with pytest.raises(E, match="square"):
        pp.GmresPolynomialOperator(sp.csr_matrix(np.ones((3, 4))), [1.0])
    with pytest.raises(E, match="degree"):
        pp.gmres_polynomial_roots(A, degree=0)
    with pytest.raises(E, match="conjugation"):
        pp.GmresPolynomialOperator(A, [1.0 + 1.0j])
    with pytest.raises(NotImplementedError, match="real operators on real blocks only"):
        pp.GmresPolynomialOperator(A.astype(complex), [1.0])
    with pytest.raises(NotImplementedError, match="real operators on real blocks only"):
        pp.gmres_polynomial_operator(A.astype(complex))
    # a singular H_d: the cyclic shift from e_1, H_2 = [[0, 0], [1, 0]]
    P = sp.csr_matrix(np.roll(np.eye(5), 1, axis=0))
    v = np.zeros((5, 1))
    v[0] = 1.0
    with pytest.raises(E, match="singular"):
        pp.gmres_polynomial_roots(P, degree=2, v=v)
    # a complex block
    op = pp.GmresPolynomialOperator(A, ROOTS["lin2"])
    with pytest.raises(utils.LinearOperatorError, match="complex device block"):
        op.dot(np.ones((20, 1), dtype=complex))


LEJA_SET = [0.3, 2.0 + 1.0j, 2.0 - 1.0j, 5.0, 1.0, 4.0 + 0.25j, 4.0 - 0.25j, 2.0, 2.0, 0.1 + 3.0j, 0.1 - 3.0j, -5.0]


def case_leja():
    """A fixed 12-root set with a repeated root and two roots of the same modulus: the package's order is the oracle's."""
    from krypy_amd import polyprecond as pp

    got = pp._leja(np.array(LEJA_SET, dtype=complex))
    want = ref.leja_ref(LEJA_SET)
    assert np.array_equal(got, want)
    assert got[0] == 5.0 and sorted(got, key=lambda t: (t.real, t.imag)) == sorted(
        np.array(LEJA_SET, dtype=complex), key=lambda t: (t.real, t.imag))
    for i, t in enumerate(got):
        if t.imag > 0:
            assert got[i + 1] == t.conjugate()


# ---- the operator -----------------------------------------------------------------------------------------------------------
def case_attributes():
    from krypy_amd import polyprecond as pp
    from krypy_amd import utils

    A = bc.convdiff(6, 4, 0.5, 0.25)
    op = utils.gmres_polynomial_operator(A, degree=5, seed=1)
    assert utils.gmres_polynomial_operator is pp.gmres_polynomial_operator
    assert isinstance(op, pp.GmresPolynomialOperator) and op._device_matrix() is None
    assert op.degree == 5 and op.roots.shape == (5,) and op.steps.shape == (4, 5) and op.info["degree"] == 5
    assert op.info["log10_pof_max"] == ref.log10_pof_max_ref(op.roots) and op.info["log10_pof_max"] < 4
    assert op.shape == (24, 24) and op.dtype == np.float64
    assert "GmresPolynomialOperator" in repr(op) and "degree 5" in repr(op)
    v = np.random.default_rng(1).standard_normal((24, 1))
    roots, info = pp.gmres_polynomial_roots(A, degree=5, v=v)
    assert np.array_equal(roots, op.roots) and info == op.info
    assert "gmres_polynomial_operator" not in utils.__all__


def case_residual_polynomial(degree, start=False):
    """``|w - A p(A) w| / |w|`` equals ``|pi(A) w| / |w|``, ``pi(z) = prod (1 - z / theta_i)``, evaluated from a dense
    eigendecomposition of the 24-row matrix.  ``w``: a seeded vector, or - ``start`` - the start vector of the Arnoldi steps
    (then the value is the GMRES residual after ``degree`` steps, which falls with the degree)."""
    from krypy_amd import utils

    A = bc.convdiff(6, 4, 0.5, 0.25)
    n = A.shape[0]
    op = utils.gmres_polynomial_operator(A, degree=degree)
    w = np.random.default_rng(0 if start else 3).standard_normal((n, 1))
    lhs = np.linalg.norm(w - A.dot(op.dot(w))) / np.linalg.norm(w)
    lam, V = np.linalg.eig(A.toarray())
    pi = np.ones(n, dtype=complex)
    for t in op.roots:
        pi = pi * (1 - lam / t)
    rhs = np.linalg.norm(V @ (pi * np.linalg.solve(V, w[:, 0].astype(complex)))) / np.linalg.norm(w)
    print("degree %d: |w - A p(A) w| / |w| = %.17g, from the eigendecomposition %.17g" % (degree, lhs, rhs))
    assert abs(lhs - rhs) <= RTOL_RESIDUAL * rhs
    return lhs


def case_invariant_subspace():
    """Three distinct eigenvalues and a start vector with one component in each eigenspace: the subspace is invariant after
    three steps, the roots are the eigenvalues and p(A) = A^-1."""
    from krypy_amd import utils

    d = np.array([1.0, 2.0, 4.0] * 5)
    A = sp.diags(d).tocsr() + sp.csr_matrix(([1e-300], ([0], [1])), shape=(15, 15))      # (not a diagonal operator)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        op = utils.gmres_polynomial_operator(A, degree=8, v=np.concatenate((np.ones(3), np.zeros(12))))
    assert op.info["degree"] == 3 and op.degree == 3 and op.steps.shape[0] == 2
    assert np.allclose(np.sort(op.roots.real), [1.0, 2.0, 4.0], rtol=1e-12) and np.all(op.roots.imag == 0)
    b = np.arange(1.0, 16.0).reshape(-1, 1)
    assert np.allclose(op.dot(b), b / d[:, None], rtol=1e-10)


def case_unreliable_degree_warns():
    """Roots over four orders of magnitude in modulus: log10 pof > 4, and the function says so."""
    from krypy_amd import polyprecond as pp

    A = sp.diags(np.logspace(0.0, 6.0, 12)).tocsr() + sp.csr_matrix(([1e-300], ([0], [1])), shape=(12, 12))
    with pytest.warns(UserWarning, match="unreliable at this degree"):
        _, info = pp.gmres_polynomial_roots(A, degree=10)
    print("log10 pof = %.3f" % info["log10_pof_max"])
    assert info["log10_pof_max"] > 4


def case_in_place(ctx):
    from krypy_amd import utils

    A = bc.convdiff(5, 4, 0.5, 0.25)
    for name in ("lin1", "r-pair-r"):
        op = utils.GmresPolynomialOperator(A, ROOTS[name])
        b = np.random.default_rng(2).standard_normal((20, 2))
        X = ctx.upload(b)
        op._apply_dev(X, 0, X, 0, 2)
        assert np.array_equal(X.download(), ref.poly_apply_ref(A, b, op.steps)), name


class BB(object):
    """B (B z) on host arrays, the product formed as the composite operator forms it"""
    dtype = np.dtype(float)

    def __init__(self, B):
        self.B = B
        self.shape = B.shape

    def dot(self, z):
        return self.B.dot(self.B.dot(z))


def case_generic(n, name, count):
    """A given as a product of two operators (B * B) goes through ``A._apply_dev`` + ``poly_update``: the oracle's bits with
    the product formed the same way.  ``count(key)`` reads the context's counter."""
    from krypy_amd import utils

    B = (nonsym1d(n) - 0.5 * sp.identity(n)).tocsr()
    gen = utils.GmresPolynomialOperator(utils.MatrixLinearOperator(B) * utils.MatrixLinearOperator(B), ROOTS[name])
    b = np.random.default_rng(4).standard_normal((n, 2))
    c0 = [count(k) for k in ("poly_update", "poly_apply")]
    yg = gen.dot(b)
    c1 = [count(k) for k in ("poly_update", "poly_apply")]
    assert np.array_equal(yg.view(np.int64), ref.poly_apply_ref(BB(B), b, gen.steps).view(np.int64)), name
    assert [y - x for x, y in zip(c0, c1)] == [2 * gen.steps.shape[0], 0], name
    # the same A as one matrix: B (B z) and (B B) z round differently
    ym = utils.GmresPolynomialOperator((B @ B).tocsr(), ROOTS[name]).dot(b)
    assert np.linalg.norm(yg - ym) <= 1e-13 * np.linalg.norm(ym), name
    return yg


# ---- roots and solvers ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_roots(name, degree=8):
    A, _ = system(name)
    return ref.roots_ref(A, degree)


def case_roots(name):
    """The roots from the installed context's Arnoldi against poly_ref's, sorted."""
    from krypy_amd import utils

    A, _ = system(name)
    roots, info = utils.gmres_polynomial_roots(A, degree=8, seed=0)
    want = reference_roots(name)
    got_s, want_s = np.sort_complex(roots), np.sort_complex(want)
    err = float(np.max(np.abs(got_s - want_s)) / np.max(np.abs(want_s)))
    print("%s: roots differ by %.3g of the largest modulus, log10 pof %.3f" % (name, err, info["log10_pof_max"]))
    assert err <= RTOL_ROOTS
    assert info["degree"] == 8 and info["log10_pof_max"] < 0.5
    if name == "central32":
        assert np.sum(roots.imag > 0) >= 1         # complex-conjugate pairs at every degree
    return roots


def gmres(A, b, maxiter=None, **prec):
    from krypy_amd import linsys

    return linsys.Gmres(linsys.LinearSystem(A, b, **prec), tol=TOL, maxiter=maxiter)


def case_iteration_cap(name):
    """``Gmres`` with ``Mr = gmres_polynomial_operator(A, degree=8, seed=0)`` takes at most a quarter of the unpreconditioned
    iterations, and the true residual is there."""
    from krypy_amd import utils

    A, b = system(name)
    plain = gmres(A, b)
    op = utils.gmres_polynomial_operator(A, degree=8, seed=0)
    pre = gmres(A, b, Mr=op)
    it0, it1 = len(plain.resnorms) - 1, len(pre.resnorms) - 1
    res = relres(A, pre.xk, b)
    print("%s: %d iterations, %d with the degree-8 polynomial; true residual %.3g" % (name, it0, it1, res))
    assert 4 * it1 <= it0
    assert res <= TOL * (1 + 1e-6)
    return it0, it1


class Twin(object):
    """The oracle as a host callable, every application counted."""

    def __init__(self, A, steps):
        from krypy_amd import utils

        self.calls = 0
        n = A.shape[0]

        def dot(X):
            self.calls += X.shape[1]
            return ref.poly_apply_ref(A, X, steps)

        self.op = utils.LinearOperator((n, n), float, dot=dot)


def run_solver(solver, key, op, maxiter=200):
    from krypy_amd import linsys, utils

    A, b = system("cd24")
    ls = linsys.LinearSystem(A, b, **{key: op})
    kw = dict(s=4) if solver == "Idrs" else {}
    try:
        sol = getattr(linsys, solver)(ls, tol=TOL, maxiter=maxiter, **kw)
    except utils.ConvergenceError as e:
        sol = e.solver
    return np.array(sol.resnorms), np.array(sol.xk)


TWINS = [("Gmres", "Ml"), ("Gmres", "Mr"), ("Bicgstab", "Mr"), ("Idrs", "Mr")]
