"""CPU tests of the ILU(0) factorisation: the oracle against independent facts, the level analysis and the greedy colouring
(hand-counted, and as the stand-alone sanitizer build of krypy_amd/csrc/ilu0.h), and the host layer (``utils.ilu0``,
``utils.ilu0_operator``) on a NumPy context whose ``ilu0`` is the oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import ilu0_cases as ic
from tests.support import tri_cases as tc
from tests.support.ilu0_ref import ilu0_ref
from tests.support.tri_ref import levels_ref, tri_solve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ilu0_double():
    from krypy_amd import _hip
    from tests.support.ilu0_numpy_context import Ilu0NumpyContext

    ctx = Ilu0NumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


# ---- the oracle against independent facts ------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_is_the_lu_factorisation_where_there_is_no_fill(cplx):
    """On a full pattern and on a tridiagonal matrix ILU(0) is the LU factorisation: L U = A (bound 1e-13 for entries of size
    <= 15 and 12 / 3 terms per entry; measured 1.8e-15 and 1.1e-16 in the real case)."""
    rng = np.random.default_rng(4)
    D = rng.uniform(-1.0, 1.0, (12, 12))
    D[np.arange(12), np.arange(12)] = np.abs(D).sum(axis=1) + 1.0
    for A in (sp.csr_matrix(D), ic.tridiagonal(200)):
        if cplx:
            A = ic.make_complex(A, 5)
        L, U, lu, bad = ilu0_ref(A)
        assert bad == -1 and lu.dtype == (np.complex128 if cplx else np.float64)
        assert abs(L.dot(U) - A).max() < 1e-13
        assert np.array_equal(L.diagonal(), np.ones(A.shape[0])) and sp.triu(L, 1).nnz == 0 and sp.tril(U, -1).nnz == 0
        assert L.nnz + U.nnz == A.nnz + A.shape[0]


@pytest.mark.parametrize("name", ["random", "lap2d", "convection", "complex"])
def test_oracle_reproduces_the_matrix_on_its_pattern_only(name):
    """On a sparse pattern L U - A vanishes ON the pattern of A (the defining property of ILU(0); bound 1e-13 max|A|, measured
    9e-16) and does not off it (measured 0.29 - 0.41: the dropped fill)."""
    A = {"random": lambda: ic.random_dominant(300, 3), "lap2d": lambda: tc.lap2d(17, 13), "convection": lambda: ic.convection(17, 13),
         "complex": lambda: ic.make_complex(ic.convection(17, 13), 2)}[name]()
    L, U, lu, bad = ilu0_ref(A)
    assert bad == -1
    R = (L.dot(U) - A).tocsr()
    P = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    on = abs(R.multiply(P)).max()
    off = abs(R - R.multiply(P)).max()
    assert on < 1e-13 * abs(A).max(), on
    assert off > 1e-3, off
    assert np.abs(U.diagonal()).min() > 1.0          # far from a breakdown


def test_oracle_breakdown():
    """[[1,1,0],[1,1,1],[0,1,3]]: the pivot of row 1 is 1 - 1 * 1 = 0; the loop goes on (1 / 0 = inf, 3 - inf = -inf) and reports
    row 1.  Two independent zero pivots: the smaller row."""
    _, _, lu, bad = ilu0_ref(sp.csr_matrix(np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, 3]])))
    assert bad == 1
    assert list(lu) == [1.0, 1.0, 1.0, 0.0, 1.0, np.inf, -np.inf]
    A = ic.two_zero_pivots()          # (the zero of row 30 stays stored: the diagonal is structurally present)
    assert A[30, 30] == 0 and 30 in A.indices[A.indptr[30]: A.indptr[31]]
    lev, _ = levels_ref(ic.strict_lower(A), True)
    assert (lev[15], lev[30]) == (2, 1)
    _, _, lu, bad = ilu0_ref(A)
    assert bad == 15 and lu[A.indptr[15] + 1] == 0.0 and lu[A.indptr[30]] == 0.0
    with pytest.raises(ValueError):
        ilu0_ref(sp.csr_matrix(np.array([[1.0, 1], [1, 0]])))


# ---- levels and colouring, hand-counted ----------------------------------------------------------------------------------
def _levels(A):
    return levels_ref(ic.strict_lower(A), True)[1]


def _multicolor(A):
    from krypy_amd import _hip

    G = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    G = (G + G.T).tocsr()
    G.sort_indices()
    color, nc = _hip.multicolor(G)
    return color, nc, np.argsort(color, kind="stable")


def test_levels_hand_counted():
    assert list(_levels(ic.tridiagonal(50))) == [1] * 50
    assert list(_levels(sp.diags(np.arange(1.0, 31.0)).tocsr())) == [30]
    cnt = _levels(tc.lap2d(37, 23))
    assert len(cnt) == 59 and cnt.max() == 23
    cnt = _levels(tc.lap2d(37, 23, "redblack"))
    assert list(cnt) == [426, 425]


@pytest.mark.parametrize("nx,ny", [(37, 23), (100, 90)])
@pytest.mark.parametrize("conv", [False, True])
def test_multicolor_is_red_black_on_the_five_point_stencil(nx, ny, conv):
    """kh_multicolor (host code of the library, no device): 2 colours and exactly the permutation of lap2d(.., "redblack"); the
    reordered matrix has 2 levels in L and in U."""
    A = ic.convection(nx, ny) if conv else tc.lap2d(nx, ny)
    color, nc, perm = _multicolor(A)
    assert nc == 2 and color.dtype == np.int32
    assert np.array_equal(perm, ic.redblack_permutation(nx, ny))
    B = A[perm][:, perm].tocsr()
    if not conv:
        assert abs(B - tc.lap2d(nx, ny, "redblack")).max() == 0
    assert len(levels_ref(tc.triangle(B, True, strict=True), True)[1]) == 2
    assert len(levels_ref(tc.triangle(B, False, strict=True), False)[1]) == 2


def test_multicolor_nine_point_and_errors():
    from krypy_amd import _hip

    A = ic.nine_point(19, 14)
    color, nc, perm = _multicolor(A)
    assert nc == 4
    C = A.tocoo()
    off = C.row != C.col
    assert not np.any(color[C.row[off]] == color[C.col[off]])       # no stored off-diagonal entry joins two rows of one colour
    # greedy, restated: the smallest colour no already-coloured neighbour holds
    want = np.full(A.shape[0], -1)
    for i in range(A.shape[0]):
        nb = A.indices[A.indptr[i]: A.indptr[i + 1]]
        used = set(want[nb[nb < i]])
        want[i] = next(c for c in range(len(used) + 1) if c not in used)
    assert np.array_equal(color, want)
    assert _hip.multicolor(sp.identity(5, format="csr"))[1] == 1
    G = sp.csr_matrix((3, 3))
    G.indptr, G.indices, G.data = np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 7, 1], dtype=np.int32), np.ones(3)
    with pytest.raises(_hip.BackendError) as e:
        _hip.multicolor(G)
    assert "status -2" in str(e.value) and "out of range in row 1" in str(e.value)


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
    """krypy_amd/csrc/ilu0.h is plain C++: compiled alone into a program with its own main (tests/support/ilu0_analysis_main.cpp)
    with -fsanitize=address,undefined and run on the CPU as a child process.  For every case and narrow_rows = 0 / 64 / 1024 the
    program walks the plan in launch order (factor_host, real and complex values) and compares the bits with the plain row-by-row
    loop; it also checks the colourings."""
    exe = str(tmp_path / "ilu0_analysis")
    subprocess.check_call(_compiler() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "krypy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "ilu0_analysis_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    got, colours = {}, {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        if rest.startswith("colors="):
            head, order = rest.split(" order ")
            colours[name] = (dict(kv.split("=") for kv in head.split()), [int(v) for v in order.split()])
        else:
            got[name] = rest if rest.startswith("refused") else dict(kv.split("=") for kv in rest.split())

    def num(name, narrow):
        g = got["%s/%d" % (name, narrow)]
        assert g["factor"] == "ok", (name, narrow, g)
        return tuple(int(g[k]) for k in ("levels", "widest", "longest", "wide", "narrow", "bad"))

    for name in ("dense12", "tridiagonal", "diagonal", "long_row", "breakdown3", "two_zero_pivots", "lap2d_natural", "lap2d_multicolor",
                 "convection_natural", "convection_multicolor", "nine_point_natural", "nine_point_multicolor"):
        for narrow in (0, 64, 1024):
            num(name, narrow)
    assert num("dense12", 1024) == (12, 1, 12, 0, 1, -1)
    assert num("tridiagonal", 1024) == (300, 1, 3, 0, 1, -1) and num("tridiagonal", 0) == (300, 1, 3, 300, 0, -1)
    assert num("diagonal", 1024) == (1, 300, 1, 0, 1, -1) and num("diagonal", 64) == (1, 300, 1, 1, 0, -1)
    assert num("long_row", 64)[:3] == (300, 1, 203)
    assert num("breakdown3", 0)[5] == 1 and num("breakdown3", 1024)[5] == 1
    assert num("two_zero_pivots", 0)[5] == 7 and num("two_zero_pivots", 64)[5] == 7
    for name in ("lap2d", "convection"):
        assert num(name + "_natural", 1024) == (59, 23, 5, 0, 1, -1) and num(name + "_natural", 0)[3:5] == (59, 0)
        assert num(name + "_multicolor", 1024) == (2, 426, 5, 0, 1, -1) and num(name + "_multicolor", 64) == (2, 426, 5, 2, 0, -1)
        head, order = colours[name + "_colouring"]
        assert head == {"colors": "2", "valid": "ok"} and order == list(ic.redblack_permutation(37, 23))
    head, order = colours["nine_point_colouring"]
    assert head == {"colors": "4", "valid": "ok"} and sorted(order) == list(range(19 * 14))
    # four colours in the order the greedy pass meets them, (ix, iy) even-even, even-odd, odd-even, odd-odd: 70, 70, 63, 63 rows
    # (10 x 7, 10 x 7, 9 x 7, 9 x 7 grid points) - with 64 two wide levels and one narrow run of two
    assert num("nine_point_multicolor", 64) == (4, 70, 9, 2, 1, -1)
    for name, word in (("unsorted", "unsorted column indices in row 1"), ("duplicate", "duplicate column indices in row 1"),
                       ("out_of_range", "column 300 out of range in row 1"), ("missing_diagonal", "row 7 has no diagonal entry")):
        assert got[name].startswith("refused") and word in got[name], (name, got[name])


# ---- the Python layer on the NumPy context -------------------------------------------------------------------------------
def test_argument_errors(ilu0_double):
    from krypy_amd import utils

    A = ic.convection(7, 5)
    with pytest.raises(utils.ArgumentError):
        utils.ilu0(A, ordering="rcm")
    with pytest.raises(utils.ArgumentError):
        utils.ilu0(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(utils.ArgumentError):
        utils.ilu0(np.ones(4))
    M = A.tolil()
    M[11, 11] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    for ordering in ("natural", "multicolor"):
        with pytest.raises(utils.ArgumentError) as e:
            utils.ilu0(M, ordering)
        assert "row 11" in str(e.value)
    assert ilu0_double.calls.get("ilu0", 0) == 0       # all refused before anything reaches the device


def test_breakdown_is_an_argument_error(ilu0_double):
    from krypy_amd import utils

    B = np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, 3]])
    with pytest.raises(utils.ArgumentError) as e:
        utils.ilu0(B)
    assert "ILU(0) breaks down: zero or non-finite pivot in row 1" in str(e.value)
    with pytest.raises(utils.ArgumentError) as e:
        utils.ilu0_operator(sp.csr_matrix(B))
    assert "pivot in row 1" in str(e.value)
    # two independent zero pivots: the smaller row is reported; under the multicolour ordering also in the original numbering
    A = ic.two_zero_pivots()
    with pytest.raises(utils.ArgumentError) as e:
        utils.ilu0(A)
    assert "pivot in row 15" in str(e.value) and "original" not in str(e.value)
    with pytest.raises(utils.ArgumentError) as e:
        utils.ilu0(A, "multicolor")
    perm = _multicolor(A)[2]
    bad = ilu0_ref(A[perm][:, perm].tocsr())[3]          # the reordered matrix is another factorisation: its own first broken row
    assert bad >= 0 and "pivot in row %d (row %d of the original numbering)" % (bad, perm[bad]) in str(e.value)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_factors_operator_and_solve(ilu0_double, ordering, cplx):
    """Both orderings: the object quacks like spilu's, passes through ilu_operator unchanged, and ilu0_operator(A).dot(b) is
    x[p] = U^{-1} L^{-1} b[p] with the oracle's substitutions, bit for bit."""
    from krypy_amd import utils

    A = ic.convection(13, 9)
    if cplx:
        A = ic.make_complex(A, 7)
    n = A.shape[0]
    f = utils.ilu0(A, ordering)
    p = ic.redblack_permutation(13, 9) if ordering == "multicolor" else np.arange(n)
    Ap = A[p][:, p].tocsr()
    L, U, lu, bad = ilu0_ref(Ap)
    assert bad == -1
    for got, want in ((f.L, L), (f.U, U)):
        got = sp.csr_matrix(got)
        assert got.has_sorted_indices and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert np.array_equal(got.data, want.data) and got.dtype == want.dtype
    assert np.array_equal(f.L.diagonal(), np.ones(n))
    assert f.shape == (n, n) and f.nnz == L.nnz + U.nnz
    assert f.info["ordering"] == ordering and f.info["colors"] == (2 if ordering == "multicolor" else None)
    assert f.info["first_broken_row"] == -1 and f.info["n"] == n and f.info["nnz"] == A.nnz
    assert f.info["levels"] == (2 if ordering == "multicolor" else 13 + 9 - 1)
    rng = np.random.default_rng(3)
    b = rng.standard_normal((n, 2)) + (1j * rng.standard_normal((n, 2)) if cplx else 0)
    want = np.zeros_like(b)
    want[p] = tri_solve_ref(U, tri_solve_ref(L, b[p], True, True), False)
    # ilu_operator's documented convention with the object's permutations gives exactly that
    y = np.zeros_like(b)
    y[f.perm_r] = b
    assert np.array_equal(y, b[p])
    op = utils.ilu_operator(f)
    assert np.array_equal(op.dot(b), want)
    assert np.array_equal(utils.ilu0_operator(A, ordering).dot(b), want)
    assert np.array_equal(f.solve(b), want)
    x1 = f.solve(b[:, 0])
    assert x1.shape == (n,) and np.array_equal(x1, want[:, 0])
    x = utils.DVec.from_host(b[:, [0]])
    assert np.array_equal((op * x).download(), want[:, [0]])
    if ordering == "natural":          # the identity permutations are left out: two factors only
        assert isinstance(op, utils._ProductLinearOperator) and all(isinstance(a, utils.TriangularSolveOperator) for a in op.args)


def test_inputs_and_widening(ilu0_double):
    """A SciPy matrix of any format, a dense array and a MatrixLinearOperator give the same factors; duplicates are summed,
    stored zeros stay in the pattern; a real fp32 input is widened to fp64, a complex64 one to complex128."""
    from krypy_amd import utils

    A = ic.convection(6, 5)
    ref = utils.ilu0(A)
    for B in (A.tocsc(), A.tocoo(), A.toarray(), utils.MatrixLinearOperator(A)):
        f = utils.ilu0(B)
        assert np.array_equal(f.L.toarray(), ref.L.toarray()) and np.array_equal(f.U.toarray(), ref.U.toarray())
    C = A.tocoo()
    dup = sp.coo_matrix((np.concatenate([C.data[::-1] * 0.5, C.data[::-1] * 0.5]), (np.concatenate([C.row[::-1]] * 2),
                                                                                  np.concatenate([C.col[::-1]] * 2))), shape=A.shape)
    f = utils.ilu0(dup)
    assert np.array_equal(f.U.toarray(), ref.U.toarray())
    # a stored zero stays in the pattern: it receives fill that eliminate_zeros would have dropped
    Z = (A + sp.csr_matrix(([1.0], ([7], [1])), shape=A.shape)).tocsr()
    Z.sort_indices()
    Z.data[(Z.indices == 1) & (np.repeat(np.arange(30), np.diff(Z.indptr)) == 7)] = 0.0
    f = utils.ilu0(Z)
    assert f.L.nnz + f.U.nnz == A.nnz + 1 + 30 and f.L[7, 1] == 0.0 and f.U[7, 7] == ref.U[7, 7]
    f32 = utils.ilu0(A.astype(np.float32))
    assert f32.L.dtype == np.float64 and f32.U.dtype == np.float64
    assert np.array_equal(f32.U.toarray(), utils.ilu0(A.astype(np.float32).astype(np.float64)).U.toarray())
    assert utils.ilu0(A.astype(np.complex64)).U.dtype == np.complex128
    assert utils.ilu0_operator(A.astype(np.float32)).dtype == np.float64
