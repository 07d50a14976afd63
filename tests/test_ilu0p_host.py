"""CPU tests of the persistent ILU(0) preconditioner: the oracle (tests/support/ilu0p_ref.py) against independent facts, the
host analysis and the row arithmetic of krypy_amd/csrc/ilu0p.h as a stand-alone sanitizer build, and the Python layer
(``utils.Ilu0Preconditioner``) on a NumPy context whose ``ilu0_handle`` / ``ilu0_refactor`` / ``ilu0_solve`` are the oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import ilu0_cases as ic
from tests.support.ilu0_ref import ilu0_ref
from tests.support.ilu0p_ref import Ilu0pRef, permuted
from tests.support.poison import bits_equal
from tests.support.tri_ref import tri_solve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ilu0p_double():
    from krypy_amd import _hip
    from tests.support.ilu0p_numpy_context import Ilu0pNumpyContext

    ctx = Ilu0pNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


def _rhs(n, k, cplx, seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, k))
    return b + 1j * rng.standard_normal((n, k)) if cplx else b


# ---- the oracle against independent facts ------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "redblack", "random"])
def test_oracle_is_ilu0_ref_tri_ref_and_explicit_permutations(ordering, cplx):
    A = ic.convection(9, 7)
    if cplx:
        A = ic.make_complex(A, 2)
    n = A.shape[0]
    p = {"natural": None, "redblack": ic.redblack_permutation(9, 7), "random": np.random.default_rng(5).permutation(n)}[ordering]
    ref = Ilu0pRef(A, p)
    q = np.arange(n) if p is None else p
    P = sp.csr_matrix((np.ones(n), (np.arange(n), q)), shape=(n, n))          # (P v)_i = v[q_i]
    Ap = (P @ A @ P.T).tocsr()
    Ap.sort_indices()
    assert ref.Ap.has_canonical_format and abs(ref.Ap - Ap).max() == 0 and ref.Ap.nnz == A.nnz
    assert np.array_equal(ref.Ap.data, A.data[ref.src]) and np.array_equal(np.sort(ref.src), np.arange(A.nnz))
    L, U, lu, bad = ilu0_ref(Ap)
    assert bad == -1 == ref.bad
    want_values = np.empty_like(lu)
    want_values[ref.src] = lu
    bits_equal(ref.values, want_values, "values")
    # position by position: the value at the caller's entry (i, j) is the factored value of Ap at (inv[i], inv[j])
    inv = np.empty(n, dtype=np.int64)
    inv[q] = np.arange(n)
    LU = (sp.tril(L, -1) + U).tocsr()
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    assert np.array_equal(ref.values, np.asarray(LU[inv[rows], inv[A.indices]]).ravel())
    b = _rhs(n, 2, cplx, 3)
    want = P.T @ tri_solve_ref(U, tri_solve_ref(L, P @ b, True, True), False)
    assert np.array_equal(ref.solve(b), want)
    bits_equal(ref.solve(b[:, 0]), ref.solve(b)[:, 0].copy(), "one vector")


@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_solves_a_tridiagonal_system(cplx):
    """On a tridiagonal matrix ILU(0) is LU, under the natural order: the oracle's solve solves A x = b (1e-13: entries <= 3, two
    substitutions with at most 2 terms per row, condition number of order 10)."""
    A = ic.tridiagonal(200)
    if cplx:
        A = ic.make_complex(A, 5)
    b = _rhs(200, 1, cplx, 8)
    x = Ilu0pRef(A).solve(b)
    assert abs(A @ x - b).max() < 1e-13
    # a reordering that keeps the matrix tridiagonal: the reversal
    x = Ilu0pRef(A, np.arange(199, -1, -1)).solve(b)
    assert abs(A @ x - b).max() < 1e-13


def test_oracle_keeps_stored_zeros_and_reports_the_reordered_row():
    A = ic.two_zero_pivots()
    assert Ilu0pRef(A).bad == 15
    p = np.arange(40)[::-1].copy()
    Ap, src = permuted(A, p)
    assert Ap.nnz == A.nnz and Ap[39 - 30, 39 - 30] == 0 and (39 - 30) in Ap.indices[Ap.indptr[9]: Ap.indptr[10]]
    assert Ilu0pRef(A, p).bad == ilu0_ref(Ap)[3] >= 0


# ---- the host header, compiled alone -------------------------------------------------------------------------------------
def _compiler():
    """A host C++ compiler and the flags that link the sanitizer runtimes STATICALLY (clang's default; GCC needs to be told)."""
    for c in ("clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return [path]
    for c in ("g++", "c++"):
        path = shutil.which(c)
        if path:
            return [path, "-static-libasan", "-static-libubsan"]
    raise AssertionError("no host C++ compiler found for the stand-alone analysis program")


def test_host_header_standalone_under_sanitizers(tmp_path):
    """krypy_amd/csrc/ilu0p.h is plain C++: compiled alone into a program with its own main (tests/support/ilu0p_main.cpp) with
    -fsanitize=address,undefined and run on the CPU as a child process.  What the program checks per case is in its header."""
    exe = str(tmp_path / "ilu0p_main")
    subprocess.check_call(_compiler() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "krypy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "ilu0p_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    got, refused = {}, {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        if rest.startswith("refused") or rest.startswith("ACCEPTED"):
            refused[name] = rest
        else:
            got[name] = dict(kv.split("=") for kv in rest.split())

    def num(name, ordering, narrow):
        g = got["%s/%s/%d" % (name, ordering, narrow)]
        assert (g["pattern"], g["plan"], g["images"], g["solve"]) == ("ok", "ok", "ok", "ok"), (name, ordering, narrow, g)
        return tuple(int(g[k]) for k in ("levels", "levels_l", "levels_u", "wide", "narrow", "solve_wide", "solve_narrow"))

    cases = [("band%d" % n, o) for n in (1, 2, 63, 64, 65, 129, 4097) for o in ("natural", "random")]
    cases += [("random20001", "natural"), ("random20001", "multicolor"), ("convection", "natural"), ("convection", "multicolor"),
              ("nine_point", "multicolor")]
    for name, ordering in cases:
        for narrow in (0, 64, 1024):
            lev, lev_l, lev_u, wide, nar, swide, snar = num(name, ordering, narrow)
            assert lev == lev_l                      # one plan serves the factorisation and the L stage
            if narrow == 0:
                assert (wide, nar, swide, snar) == (lev_l, 0, lev_l + lev_u, 0)
    assert len(got) == 3 * len(cases)
    assert num("band1", "natural", 1024) == (1, 1, 1, 0, 1, 0, 2)
    # the 37 x 23 five-point grid: 59 anti-diagonals in the natural order, 2 colours; 426 > 64 rows per colour
    assert num("convection", "natural", 1024) == (59, 59, 59, 0, 1, 0, 2) and num("convection", "natural", 0)[5] == 118
    assert num("convection", "multicolor", 1024) == (2, 2, 2, 0, 1, 0, 2) and num("convection", "multicolor", 64) == (2, 2, 2, 2, 0, 4, 0)
    assert num("nine_point", "multicolor", 64)[:3] == (4, 4, 4)
    for name, word in (("perm_duplicate", "perm is not a permutation of 0 .. n-1 (entry 17)"),
                       ("perm_out_of_range", "perm is not a permutation of 0 .. n-1 (entry 200)"),
                       ("duplicate", "duplicate column indices in row 1"), ("unsorted", "unsorted column indices in row 1"),
                       ("missing_diagonal", "row 7 has no diagonal entry")):
        assert refused[name].startswith("refused") and word in refused[name], (name, refused[name])


# ---- the Python layer on the NumPy context -------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_preconditioner_equals_the_composed_operator_and_the_oracle(ilu0p_double, ordering, cplx):
    from krypy_amd import utils

    A = ic.convection(13, 9)
    if cplx:
        A = ic.make_complex(A, 7)
    n = A.shape[0]
    M = utils.Ilu0Preconditioner(A, ordering)
    assert utils.ilu0_preconditioner(A, ordering).ordering == ordering == M.ordering
    assert isinstance(M, utils.LinearOperator) and M.shape == (n, n) and M.dtype == A.dtype and M._device_matrix() is None
    b = _rhs(n, 3, cplx, 3)
    got = M.dot(b)
    # the composed operator's permutation products turn -0 into +0: equality of values there, bits against the oracle
    assert np.array_equal(got, utils.ilu0_operator(A, ordering).dot(b))
    p = ic.redblack_permutation(13, 9) if ordering == "multicolor" else None
    ref = Ilu0pRef(A, p)
    bits_equal(got, ref.solve(b), "dot")
    x = utils.DVec.from_host(b[:, [1]])
    bits_equal((M * x).download(), ref.solve(b[:, [1]]), "device vector")
    info = M.info
    assert (info["ordering"], info["colors"], info["refactorisations"]) == (ordering, 2 if p is not None else None, 1)
    assert info["factored"] and info["permuted"] == (p is not None) and (info["n"], info["nnz"]) == (n, A.nnz)
    assert info["levels"] == (2 if p is not None else 13 + 9 - 1)
    # no adjoint
    with pytest.raises(utils.LinearOperatorError):
        M.dot_adj(b)
    if not cplx:          # a real preconditioner meets complex vectors: a second, complex handle, factored in complex arithmetic
        z = _rhs(n, 1, True, 4)
        bits_equal(M.dot(z), Ilu0pRef(A.astype(np.complex128), p).solve(z), "complex vectors")
        assert ilu0p_double.calls["ilu0_handle"] == 3          # M, the one-liner's, and the complex image of M


def test_arguments_are_those_of_ilu0(ilu0p_double):
    from krypy_amd import utils

    A = ic.convection(7, 5)
    bad_inputs = [((A, "rcm"), "ordering"), ((sp.csr_matrix(np.ones((3, 4))),), "square"), ((np.ones(4),), "matrix expected")]
    M = A.tolil()
    M[11, 11] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    bad_inputs += [((M, o), "row 11") for o in ("natural", "multicolor")]
    for args, word in bad_inputs:
        with pytest.raises(utils.ArgumentError) as e1:
            utils.ilu0(*args)
        with pytest.raises(utils.ArgumentError) as e2:
            utils.Ilu0Preconditioner(*args)
        assert str(e1.value) == str(e2.value) and word in str(e1.value)
    assert ilu0p_double.calls.get("ilu0_handle", 0) == 0       # all refused before anything reaches the device


def test_update_refuses_another_pattern(ilu0p_double):
    from krypy_amd import utils

    A = ic.convection(7, 5)
    M = utils.Ilu0Preconditioner(A, "multicolor")
    for B, row in ((ic.without(A, [(17, 18)]), 17), (ic.without(A, [(3, 2), (20, 21)]), 3),
                   ((A + sp.csr_matrix(([1.0], ([9], [30])), shape=A.shape)).tocsr(), 9),
                   (ic.without(A + sp.csr_matrix(([1.0], ([9], [30])), shape=A.shape), [(9, 8)]), 9)):
        with pytest.raises(utils.ArgumentError) as e:
            M.update(B)
        assert "pattern differs" in str(e.value) and str(e.value).endswith("row %d" % row), str(e.value)
    with pytest.raises(utils.ArgumentError):
        M.update(ic.convection(7, 6))
    with pytest.raises(utils.ArgumentError):
        M.update(ic.make_complex(A, 1))
    # nothing of that touched the device or the object: it still applies the factors of A
    assert ilu0p_double.calls["ilu0_refactor"] == 1
    b = _rhs(35, 1, False, 2)
    bits_equal(M.dot(b), Ilu0pRef(A, ic.redblack_permutation(7, 5)).solve(b), "after refused updates")
    # a stored zero keeps the pattern: accepted
    M.update(ic.with_values(A, {(17, 18): 0.0}))
    assert ilu0p_double.calls["ilu0_refactor"] == 2


def test_breakdown_raises_blocks_and_a_good_update_revives(ilu0p_double):
    from krypy_amd import utils

    B = sp.csr_matrix(np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, 3]]))
    with pytest.raises(utils.ArgumentError) as e:
        utils.Ilu0Preconditioner(B)
    assert str(e.value) == "ILU(0) breaks down: zero or non-finite pivot in row 1"
    good = ic.with_values(ic.two_zero_pivots(), {(15, 15): 3.0, (30, 30): 2.0})
    A = ic.two_zero_pivots()
    for ordering in ("natural", "multicolor"):
        with pytest.raises(utils.ArgumentError) as e0:
            utils.ilu0(A, ordering)
        M = utils.Ilu0Preconditioner(good, ordering)
        with pytest.raises(utils.ArgumentError) as e:
            M.update(A)
        assert str(e.value) == str(e0.value)
        assert ("of the original numbering" in str(e.value)) == (ordering == "multicolor")
        b = _rhs(40, 1, False, 6)
        with pytest.raises(utils.LinearOperatorError):
            M.dot(b)
        with pytest.raises(utils.LinearOperatorError):
            M._apply_dev(ilu0p_double.upload(b), 0, ilu0p_double.alloc(40, 1), 0)
        assert not M.info["factored"]
        M.update(good)
        bits_equal(M.dot(b), utils.Ilu0Preconditioner(good, ordering).dot(b), "revived")


def test_updates_refactor_and_never_analyse_again(ilu0p_double):
    from krypy_amd import utils

    A = ic.convection(8, 6)
    M = utils.Ilu0Preconditioner(A, "multicolor")
    r0 = ilu0p_double.calls["ilu0_refactor"]
    b = _rhs(48, 1, False, 1)
    for k, wind in enumerate((1.0, 1.5, 2.0)):
        Ak = ic.convection(8, 6, wind=0.8 * wind)
        assert np.array_equal(Ak.indices, A.indices)
        M.update(Ak)
        bits_equal(M.dot(b), Ilu0pRef(Ak, ic.redblack_permutation(8, 6)).solve(b), "wind %g" % wind)
        assert M.info["refactorisations"] == 2 + k
    assert ilu0p_double.calls["ilu0_handle"] == 1 and ilu0p_double.calls["ilu0_refactor"] - r0 == 3
