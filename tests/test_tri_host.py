"""CPU tests of the sparse triangular solves: the oracle itself, the level analysis (restated in NumPy and as the stand-alone
sanitizer build of krypy_amd/csrc/tri.h), and the host layer (``utils.TriangularSolveOperator``, ``utils.ilu_operator``) on a
NumPy context whose ``tri`` / ``tri_solve`` are the oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.support import tri_cases as tc
from tests.support.tri_ref import level_order_ref, levels_ref, tri_solve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def tri_double():
    from krypy_amd import _hip
    from tests.support.tri_numpy_context import TriNumpyContext

    ctx = TriNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# ---- the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("lower", [True, False])
def test_oracle_against_spsolve_triangular(lower, unit, cplx):
    """The sequential substitution against SciPy's solver (which scales the rows first: another order of operations, measured
    1.4e-16 ... 2.4e-16 apart) at 1e-13 relative."""
    T = tc.random_triangular(400, 0.02, 5, lower=lower)
    if cplx:
        T = tc.make_complex(T, 6)
    rng = np.random.default_rng(7)
    b = rng.standard_normal((400, 2)) + (1j * rng.standard_normal((400, 2)) if cplx else 0)
    x = tri_solve_ref(T, b, lower, unit)
    Ts = T.copy()
    if unit:
        Ts.setdiag(1.0)
    want = spla.spsolve_triangular(sp.csr_matrix(Ts), b, lower=lower, unit_diagonal=unit)
    assert _rel(x, want) < 1e-13
    assert x.dtype == (np.complex128 if cplx else np.float64)


def test_oracle_complex_quotient_is_numpys():
    """The quotient the kernels use (Smith's formula: ratio and scale once) is what NumPy computes for complex128 scalars."""
    rng = np.random.default_rng(3)
    for a, d in zip(rng.standard_normal(500) + 1j * rng.standard_normal(500), rng.standard_normal(500) + 1j * rng.standard_normal(500)):
        ar, ai, dr, di = float(a.real), float(a.imag), float(d.real), float(d.imag)
        if abs(dr) >= abs(di):
            rat = di / dr
            scl = 1.0 / (dr + di * rat)
            q = complex((ar + ai * rat) * scl, (ai - ar * rat) * scl)
        else:
            rat = dr / di
            scl = 1.0 / (di + dr * rat)
            q = complex((ar * rat + ai) * scl, (ai * rat - ar) * scl)
        got = np.complex128(a) / np.complex128(d)
        assert q.real == got.real and q.imag == got.imag


@pytest.mark.parametrize("permc", ["NATURAL", "COLAMD"])
def test_ilu_convention_with_the_oracle(permc):
    """``y[perm_r] = b; z = U \\ (L \\ y); x = z[perm_c]`` with the oracle's substitutions is ``ilu.solve`` at 1e-13."""
    A = (tc.lap2d(19, 13) + sp.diags(np.linspace(0.1, 1.0, 19 * 13 - 1), 1)).tocsc()
    ilu = spla.spilu(A, drop_tol=1e-4, fill_factor=10, permc_spec=permc)
    b = np.random.default_rng(1).standard_normal(A.shape[0])
    y = np.zeros_like(b)
    y[ilu.perm_r] = b
    z = tri_solve_ref(ilu.U, tri_solve_ref(ilu.L, y, True, True), False, False)
    assert _rel(z[ilu.perm_c], ilu.solve(b)) < 1e-13


# ---- level analysis ------------------------------------------------------------------------------------------------
def test_levels_hand_counted():
    lev, cnt = levels_ref(tc.bidiagonal(50, True), True)
    assert list(cnt) == [1] * 50 and list(lev) == list(range(1, 51))
    lev, cnt = levels_ref(tc.bidiagonal(50, False), False)
    assert list(cnt) == [1] * 50 and list(lev) == list(range(50, 0, -1))
    _, cnt = levels_ref(sp.diags(np.arange(1.0, 31.0)).tocsr(), True)
    assert list(cnt) == [30]
    _, cnt = levels_ref(tc.triangle(tc.lap2d(37, 23, "redblack"), True), True)
    assert list(cnt) == [426, 425]
    _, cnt = levels_ref(tc.triangle(tc.lap2d(37, 23, "redblack"), False), False)
    assert list(cnt) == [425, 426]
    lev, cnt = levels_ref(tc.triangle(tc.lap2d(37, 23), True), True)
    assert len(cnt) == 59 and cnt.max() == 23 and cnt[0] == 1
    p = np.arange(37 * 23)
    assert np.array_equal(lev, p // 23 + p % 23 + 1)         # the anti-diagonals of the grid
    # level, then row length descending, then row index: row 4 (two entries) before rows 2 and 3 (one entry) of its level
    T = sp.csr_matrix(np.array([[1.0, 0, 0, 0, 0], [0, 1, 0, 0, 0], [1, 0, 1, 0, 0], [0, 1, 0, 1, 0], [1, 1, 0, 0, 1]]))
    assert list(level_order_ref(T, True)) == [0, 1, 4, 2, 3]


def _compiler():
    """A host C++ compiler and the flags that link the sanitizer runtimes STATICALLY (clang's default; GCC needs to be told):
    the program then does not care what else the process environment loads."""
    for c in ("clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return [path]
    for c in ("g++", "c++"):
        path = shutil.which(c)
        if path:
            return [path, "-static-libasan", "-static-libubsan"]
    raise AssertionError("no host C++ compiler found for the stand-alone analysis program")


def test_analysis_header_standalone_under_sanitizers(tmp_path):
    """krypy_amd/csrc/tri.h is plain C++: compiled alone into a program with its own main (tests/support/tri_analysis_main.cpp)
    with -fsanitize=address,undefined and run on the CPU over the hand-counted cases; the program also walks every plan in launch
    order and compares the bits with a row-by-row substitution on the CSR input."""
    exe = str(tmp_path / "tri_analysis")
    subprocess.check_call(_compiler() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "krypy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "tri_analysis_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    got, orders = {}, {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        if name == "order":
            name, rest = rest.split(" ", 1)
            orders[name] = [int(v) for v in rest.split()]
            continue
        got[name] = rest if rest.startswith("refused") else dict(kv.split("=") for kv in rest.split())
    def num(name):
        g = got[name]
        assert g["solve"] == "ok", (name, g)
        return tuple(int(g[k]) for k in ("levels", "widest", "longest", "wide", "narrow", "first"))
    assert num("natural_lower") == (59, 23, 2, 0, 1, 1)
    assert num("natural_upper") == (59, 23, 2, 0, 1, 1)
    assert num("natural_lower_wide") == (59, 23, 2, 59, 0, 1)
    # tri_narrow_rows = 16: anti-diagonals 1 .. 16 and 44 .. 59 are two narrow runs, the 27 between them wide
    assert num("natural_lower_mixed") == (59, 23, 2, 27, 2, 1)
    assert num("redblack_lower") == (2, 426, 4, 0, 1, 426)
    assert num("redblack_upper") == (2, 426, 4, 2, 0, 425)
    assert num("bidiagonal") == (300, 1, 1, 0, 1, 1)
    assert num("diagonal") == (1, 300, 0, 0, 1, 300)
    assert num("long_row")[:3] == (300, 1, 201)
    assert num("zero_diagonal_unit")[:1] == (300,)
    assert int(got["diagonal"]["slots"]) == 0
    # slices are padded to their first (longest) row.  Red rows carry nothing; of the 425 black rows the 367 interior ones have 4
    # entries and come first (the four corners are red: no row has 2), so slices 0 .. 5 start with a 4-entry row and slice 6
    # (rows 384 ..) with a 3-entry one
    assert int(got["redblack_lower"]["slots"]) == (6 * 4 + 3) * 64
    # the plan's row order is the NumPy restatement's: by level, then row length descending, then row index ascending
    longrow = tc.bidiagonal(300).tolil()
    longrow[250, :200] = 1.0
    for name, T, lower in (("natural_lower", tc.triangle(tc.lap2d(37, 23), True), True),
                           ("natural_upper", tc.triangle(tc.lap2d(37, 23), False), False),
                           ("redblack_lower", tc.triangle(tc.lap2d(37, 23, "redblack"), True), True),
                           ("redblack_upper", tc.triangle(tc.lap2d(37, 23, "redblack"), False), False),
                           ("long_row", longrow.tocsr(), True)):
        assert orders[name] == list(level_order_ref(T, lower)), name
    for name, word in (("wrong_side", "wrong side"), ("unsorted", "unsorted"), ("duplicate", "duplicate"),
                       ("zero_diagonal", "zero diagonal"), ("missing_diagonal", "no diagonal")):
        assert got[name].startswith("refused") and word in got[name], (name, got[name])


# ---- host layer on the NumPy context -------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [True, False])
def test_operator_dot_adj_and_algebra(tri_double, lower):
    from krypy_amd import utils

    n = 120
    T = tc.random_triangular(n, 0.05, 21, lower=lower)
    op = utils.TriangularSolveOperator(T)
    assert op.lower is lower and op.shape == (n, n) and op.dtype == np.float64 and op._device_matrix() is None
    rng = np.random.default_rng(2)
    X = rng.standard_normal((n, 3))
    want = tri_solve_ref(T, X, lower)
    assert np.array_equal(op.dot(X), want)
    assert np.array_equal(op * X, want)
    assert _rel(T.dot(op.dot(X)), X) < 1e-12
    # adjoint: the solve with T^H, the other triangle; built once
    adj = op.adj
    assert isinstance(adj, utils.TriangularSolveOperator) and adj.lower is (not lower) and op.adj is adj and adj.adj is op
    assert np.array_equal(adj.dot(X), tri_solve_ref(T.T.conj().tocsr(), X, not lower))
    assert np.array_equal(op.dot_adj(X), adj.dot(X))
    # algebra: products, sums and scalings go through _apply_dev on device vectors
    A = utils.MatrixLinearOperator(tc.lap2d(12, 10))
    x = utils.DVec.from_host(X[:, [0]])
    y = ((op * A) * x).download()
    assert _rel(y, tri_solve_ref(T, tc.lap2d(12, 10).dot(X[:, [0]]), lower)) < 1e-14
    y = ((2.0 * op + op) * x).download()
    assert _rel(y, 3.0 * want[:, [0]]) < 1e-14
    calls = tri_double.calls["tri_solve"]
    timed = utils.TimedLinearOperator(op)
    assert np.array_equal((timed * x).download(), want[:, [0]]) and tri_double.calls["tri_solve"] == calls + 1
    assert tri_double.calls["tri"] == 2          # T and its adjoint, each created once


def test_dtype_widening(tri_double):
    """A real T meeting complex vectors is created a second time as c128; a complex T widens a real host operand and
    refuses a real device block."""
    from krypy_amd import utils

    n = 60
    T = tc.random_triangular(n, 0.1, 4)
    op = utils.TriangularSolveOperator(T, lower=True)
    rng = np.random.default_rng(9)
    z = rng.standard_normal((n, 1)) + 1j * rng.standard_normal((n, 1))
    assert np.array_equal(op.dot(z), tri_solve_ref(T.astype(complex), z, True))
    op.dot(z.real)
    op.dot(z)
    assert tri_double.calls["tri"] == 2
    Tz = tc.make_complex(T, 5)
    opz = utils.TriangularSolveOperator(Tz)
    assert opz.dtype == np.complex128
    assert np.array_equal(opz.dot(z.real), tri_solve_ref(Tz, z.real.astype(complex), True))
    assert np.array_equal(opz.adj.dot(z), tri_solve_ref(Tz.conj().T.tocsr(), z, False))
    with pytest.raises(utils.LinearOperatorError):
        opz._apply_dev(tri_double.upload(z.real), 0, tri_double.alloc(n, 1), 0, 1)
    # the operator advertises what the device works in: fp64 / c128 whatever came in
    for src, dst in ((np.float32, np.float64), (np.complex64, np.complex128), (np.longdouble, np.float64), (np.int64, np.float64)):
        assert utils.TriangularSolveOperator(T.astype(src)).dtype == np.dtype(dst)
    # unit diagonal: a stored diagonal is ignored
    opu = utils.TriangularSolveOperator(T, unit_diagonal=True)
    Tu = T.copy()
    Tu.setdiag(1.0)
    assert np.array_equal(opu.dot(z.real), tri_solve_ref(Tu, z.real, True))
    # unsorted input with duplicates is made canonical
    C = T.tocoo()
    dup = sp.coo_matrix((np.concatenate([C.data[::-1] * 0.5, C.data[::-1] * 0.5]), (np.concatenate([C.row[::-1]] * 2),
                                                                                  np.concatenate([C.col[::-1]] * 2))), shape=T.shape)
    assert _rel(utils.TriangularSolveOperator(dup).dot(z.real), op.dot(z.real)) < 1e-14


def test_argument_errors(tri_double):
    from krypy_amd import utils

    T = tc.random_triangular(30, 0.2, 8)
    full = (T + T.T).tocsr()
    with pytest.raises(utils.ArgumentError):
        utils.TriangularSolveOperator(full)
    with pytest.raises(utils.ArgumentError):
        utils.TriangularSolveOperator(T, lower=False)
    with pytest.raises(utils.ArgumentError):
        utils.TriangularSolveOperator(T.T.tocsr(), lower=True)
    with pytest.raises(utils.ArgumentError):
        utils.TriangularSolveOperator(tc.random_triangular(30, 0.2, 8, diag=False))          # missing diagonal
    Z = T.tolil()
    Z[4, 4] = 0.0
    with pytest.raises(utils.ArgumentError):
        utils.TriangularSolveOperator(Z.tocsr())                                              # zero diagonal
    utils.TriangularSolveOperator(tc.random_triangular(30, 0.2, 8, diag=False), lower=True, unit_diagonal=True)
    with pytest.raises(utils.ArgumentError):
        utils.TriangularSolveOperator(sp.csr_matrix(np.ones((3, 4))))
    assert tri_double.calls.get("tri", 0) == 0       # all refused (or not yet needed) before anything reaches the device


@pytest.mark.parametrize("permc", ["NATURAL", "COLAMD"])
def test_ilu_operator(tri_double, permc):
    from krypy_amd import utils

    A = (tc.lap2d(19, 13) + sp.diags(np.linspace(0.1, 1.0, 19 * 13 - 1), 1)).tocsc()
    n = A.shape[0]
    ilu = spla.spilu(A, drop_tol=1e-4, fill_factor=10, permc_spec=permc, diag_pivot_thresh=0.0 if permc == "NATURAL" else 1.0)
    op = utils.ilu_operator(ilu)
    b = np.random.default_rng(1).standard_normal((n, 2))
    assert _rel(op.dot(b), ilu.solve(b)) < 1e-13
    x = utils.DVec.from_host(b[:, [0]])
    assert _rel((op * x).download(), ilu.solve(b[:, 0]).reshape(-1, 1)) < 1e-13
    ident = np.array_equal(ilu.perm_r, np.arange(n)) and np.array_equal(ilu.perm_c, np.arange(n))
    assert ident == (permc == "NATURAL")
    # the identity permutations are left out: two factors only
    nfac = 0
    stack = [op]
    while stack:
        o = stack.pop()
        if isinstance(o, utils._ProductLinearOperator):
            stack += list(o.args)
        else:
            nfac += 1
    assert nfac == (2 if ident else 4)
    # adjoint of the product through the factors' adjoints
    assert _rel(op.dot_adj(b), ilu.solve(b, "H")) < 1e-13


def test_gmres_with_ilu_against_recorded_reference(tri_double, golden):
    """The reference's GMRES with ``Ml = LinearOperator(ilu.solve)`` (tools/gen_tri_golden.py) against the host layer with
    ``ilu_operator`` of the stored factors, at the project's 1e-10 bar (the last entry is an explicitly formed residual)."""
    from krypy_amd import linsys, utils

    g = golden("tri_precond")
    n = int(g["n"])

    class Factors(object):
        L, U = (sp.csr_matrix((g[t + "_data"], g[t + "_indices"], g[t + "_indptr"]), shape=(n, n)) for t in "LU")
        perm_r, perm_c = g["perm_r"], g["perm_c"]

    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(n, n))
    sol = linsys.Gmres(linsys.LinearSystem(A, g["b"], Ml=utils.ilu_operator(Factors)), tol=1e-8, maxiter=100)
    got, want = np.array(sol.resnorms), g["resnorms"]
    assert got.shape == want.shape
    assert np.max(np.abs(got[:-1] - want[:-1]) / want[:-1]) < 1e-10
    assert _rel(sol.xk, g["xk"]) < 1e-10
    assert tri_double.calls["tri_solve"] >= 2 * (len(want) - 1)
