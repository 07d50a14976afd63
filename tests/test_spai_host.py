"""CPU tests of the sparse approximate inverse on a fixed pattern: the oracle (tests/support/spai_ref.py) against independent
facts, krypy_amd/csrc/spai.h as a stand-alone sanitizer build, and the host layer (``utils.spai``, ``utils.spai_operator``) on a
NumPy context whose ``spai`` is the oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import spai_cases as sc
from tests.support.spai_ref import pattern_of, spai_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture
def spai_double():
    from krypy_amd import _hip
    from tests.support.spai_numpy_context import SpaiNumpyContext

    ctx = SpaiNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


def _defect(M, A):
    """|| I - M A ||_F"""
    return np.linalg.norm(np.eye(A.shape[0]) - (M @ A).toarray())


# ---- the oracle against independent facts ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lap_A", "lap_A2", "conv_A", "conv_A2", "shifted_A", "shifted_A2"])
def test_oracle_rows_are_the_least_squares_solutions(name):
    """Row i of M solves min || A[J, :]^T m - e_i ||_2: compared with numpy.linalg.lstsq on the dense A[J, :]^T (an orthogonal
    factorisation, no normal equations).  Bar: 64 eps cond(G_row) relative to the row's largest entry, cond(G_row) computed here
    from the row's own Gram matrix (measured: cond <= 6.1 / 30 for the pattern of A / A^2 on the Laplacian, error <= 6e-15)."""
    A, P, M, bad = sc.oracle(name)
    assert bad == -1
    _, _, grams = spai_ref(A, P, want_gram=True)
    D = A.toarray()
    n = A.shape[0]
    worst = 0.0
    for i in range(n):
        J = P.indices[P.indptr[i]: P.indptr[i + 1]]
        e = np.zeros(n, dtype=D.dtype)
        e[i] = 1.0
        want = np.linalg.lstsq(D[J, :].T, e, rcond=None)[0]
        got = M.data[P.indptr[i]: P.indptr[i + 1]]
        err = np.abs(got - want).max() / np.abs(want).max()
        bar = 64 * EPS * np.linalg.cond(grams[i])
        worst = max(worst, err / bar)
        assert err <= bar, (i, err, bar)
    assert 0 < worst <= 1


@pytest.mark.parametrize("op", ["lap", "conv", "shifted"])
def test_oracle_beats_jacobi_and_the_larger_pattern_beats_the_smaller(op):
    """|| I - M A ||_F: SPAI on the pattern of A below diag(A)^{-1} (the best DIAGONAL matrix is itself a feasible point of the
    larger problem), the pattern of A^2 below the pattern of A (a superset).  37 x 23 Laplacian: 14.3, 8.07, 5.75."""
    A, _, M1, _ = sc.oracle(op + "_A")
    _, _, M2, _ = sc.oracle(op + "_A2")
    jac = _defect(sp.diags(1.0 / A.diagonal()).tocsr(), A)
    d1, d2 = _defect(M1, A), _defect(M2, A)
    assert d2 < d1 < jac, (d2, d1, jac)
    if op == "lap":
        assert abs(jac - 14.3) < 0.05 and abs(d1 - 8.07) < 0.005 and abs(d2 - 5.75) < 0.005


@pytest.mark.parametrize("name", ["lap_A", "conv_A2", "shifted_A"])
def test_oracle_is_a_minimum_on_its_pattern(name):
    """Twenty seeded random perturbations of M on the same pattern (relative size 1e-3): none has a smaller || I - M A ||_F."""
    A, P, M, _ = sc.oracle(name)
    best = _defect(M, A)
    rng = np.random.default_rng(8)
    for _ in range(20):
        E = rng.standard_normal(M.nnz) + (1j * rng.standard_normal(M.nnz) if M.dtype.kind == "c" else 0)
        Mp = sp.csr_matrix((M.data + 1e-3 * np.abs(M.data).max() * E, P.indices, P.indptr), shape=M.shape)
        assert _defect(Mp, A) >= best


def test_oracle_exact_cases():
    d = np.linspace(0.5, 4.0, 9) * np.array([1, -1, 1, 1, -1, 1, 1, 1, -1])
    M, bad = spai_ref(sp.diags(d).tocsr())
    assert bad == -1 and M.nnz == 9 and np.allclose(M.diagonal() * d, 1.0, rtol=4 * EPS, atol=0)
    rng = np.random.default_rng(2)
    for cplx in (False, True):
        D = rng.standard_normal((6, 6)) + 3.0 * np.eye(6) + (0.5j * rng.standard_normal((6, 6)) if cplx else 0)
        M, bad = spai_ref(sp.csr_matrix(D), np.ones((6, 6)))
        assert bad == -1 and np.abs(M.toarray() @ D - np.eye(6)).max() < 1e-12
    # side="right" restated: the transposes are plain
    A = sc.complex_shifted(5, 4)
    Mr = spai_ref(A.T.tocsr())[0].T.tocsr()
    Ml = spai_ref(A)[0]
    n = A.shape[0]
    assert np.linalg.norm(np.eye(n) - (A @ Mr).toarray()) < np.linalg.norm(np.eye(n) - (A @ Ml).toarray())


def test_oracle_breakdowns():
    """Exact by construction: d = 0 comes out of g - (g / g) g and of a sum of zeros, whatever the rounding."""
    A, P, M, bad = sc.oracle("identical_rows")
    assert bad == 3 and np.array_equal(A[3].toarray(), A[4].toarray())
    rows = np.repeat(np.arange(12), np.diff(P.indptr))
    broken = np.unique(rows[~np.isfinite(M.data)])
    assert list(broken) == [3, 4]          # the loop went on: the other rows are finite
    A, P, M, bad = sc.oracle("zero_row")
    assert bad == 8 and A[9].nnz == 5 and abs(A[9]).max() == 0
    assert list(np.unique(rows[~np.isfinite(M.data)])) == [8, 9, 10]
    assert sc.oracle("two_broken_rows")[3] == 3
    assert sc.oracle("zzero_row")[3] == 8


# ---- krypy_amd/csrc/spai.h alone, under the host sanitizers ----------------------------------------------------------------
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
    raise AssertionError("no host C++ compiler found for the stand-alone program")


def test_header_standalone_under_sanitizers(tmp_path):
    """krypy_amd/csrc/spai.h is plain C++: compiled alone into a program with its own main (tests/support/spai_main.cpp) with
    -fsanitize=address,undefined and run on the CPU as a child process.  For every case, real and complex, the program computes
    all rows with a plain sequential loop of its own and with the header's row routine on 1 / 8 / 16 / 32 / 64 emulated lanes -
    the split the kernel makes - and compares the bits; then it feeds the validation every kind of bad input."""
    exe = str(tmp_path / "spai_main")
    subprocess.check_call(_compiler() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "krypy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "spai_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    runs, refused = {}, {}
    for line in r.stdout.splitlines():
        name, rest = line.split(" ", 1)
        if rest.startswith("refused: "):
            refused[name] = rest[len("refused: "):]
        else:
            runs[name] = dict(kv.split("=") for kv in rest.split())
    want_q = {"grid_pattern_A": 5, "grid_pattern_A2": 13, "band_q31": 31, "band_q32": 32, "no_diagonal_empty_row": 4, "breakdown": 3}
    for case, q in want_q.items():
        for kind in "rz":
            for W in (1, 8, 16, 32, 64):
                g = runs["%s/%s/%d" % (case, kind, W)]
                assert g["bits"] == "ok" and int(g["q"]) == q, (case, kind, W, g)
                assert (int(g["bad"]) >= 0) == (case == "breakdown"), (case, kind, W, g)
    assert len(runs) == len(want_q) * 2 * 5
    assert int(runs["breakdown/r/16"]["bad"]) == 3          # rows 3 and 4 of A are identical there; row 9 is zero
    for name, word in (("n_zero", "n = 0 out of range"), ("n_too_large", "n = 2147483648 out of range"),
                       ("nnz_too_large", "nnz = 2147483648 of A out of range"),
                       ("unsorted_A", "unsorted column indices in row 5 of A"),
                       ("unsorted_pattern", "unsorted column indices in row 5 of the pattern"),
                       ("duplicate_A", "duplicate column indices in row 6 of A"),
                       ("duplicate_pattern", "duplicate column indices in row 6 of the pattern"),
                       ("out_of_range_A", "column 117 out of range in row 7 of A"),
                       ("out_of_range_pattern", "column 117 out of range in row 7 of the pattern"),
                       ("negative_column", "column -1 out of range in row 2 of A"),
                       ("indptr_not_ascending", "not ascending at row 2"),
                       ("q33", "pattern row 16 has 33 entries, at most 32")):
        assert word in refused[name], (name, refused.get(name))
    assert len(refused) == 12


# ---- the Python layer on the NumPy context -------------------------------------------------------------------------------
def _same_matrix(got, want):
    got = sp.csr_matrix(got)
    assert got.has_sorted_indices and got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64))


@pytest.mark.parametrize("name", ["conv_A", "shifted_A2"])
def test_left_right_and_pattern_as_a_matrix(spai_double, name):
    from krypy_amd import utils

    A, P, want, _ = sc.oracle(name)
    given = None if name.endswith("_A") else A @ A
    M = utils.spai(A, given)
    _same_matrix(M, want)
    assert M.info["first_broken_row"] == -1 and M.info["side"] == "left" and M.info["symmetric"] is False
    assert (M.info["n"], M.info["pnnz"], M.info["qmax"]) == (A.shape[0], P.nnz, int(np.diff(P.indptr).max()))
    W = 8 if name == "conv_A" else 16          # q = 5: 8 lanes per row, 32 rows per workgroup; q = 13: 16 and 16
    assert M.info["group_width"] == W and M.info["workgroups"] == -(-A.shape[0] // (256 // W))
    # the pattern as a dense array, as a sparse matrix of another format and with other values: only the pattern is read
    if given is not None:
        for Pm in (P.toarray(), P.tocoo(), 7.0 * P):
            _same_matrix(utils.spai(A, Pm), want)
    # right: the left inverse of the plain transpose on the transposed pattern, transposed back
    Mr = utils.spai(A, given, side="right")
    wr = spai_ref(A.T.tocsr(), None if given is None else P.T.tocsr())[0].T.tocsr()
    wr.sort_indices()
    _same_matrix(Mr, wr)
    assert Mr.info["side"] == "right"
    n = A.shape[0]
    assert np.linalg.norm(np.eye(n) - (A @ Mr).toarray()) <= np.linalg.norm(np.eye(n) - (A @ M).toarray())
    op = utils.spai_operator(A, pattern=given, side="right")
    assert isinstance(op, utils.MatrixLinearOperator) and op.shape == A.shape and op.dtype == A.dtype
    _same_matrix(op._A, wr)
    assert spai_double.calls["spai"] >= 3


def test_symmetric(spai_double):
    """(M + M^H) / 2 on the host; on the 37 x 23 Laplacian it is positive definite (smallest eigenvalue 0.083) - which the
    function does not check."""
    from krypy_amd import utils

    A, P, want, _ = sc.oracle("lap_A")
    M = utils.spai(A, symmetric=True)
    assert M.info["symmetric"] is True
    S = ((want + want.conj().T) / 2).toarray()
    assert np.array_equal(M.toarray(), S) and np.array_equal(M.toarray(), M.toarray().T)
    assert abs(np.linalg.eigvalsh(S).min() - 0.083) < 5e-4
    Z, _, wz, _ = sc.oracle("shifted_A")
    Mz = utils.spai(Z, symmetric=True).toarray()
    assert np.array_equal(Mz, ((wz + wz.conj().T) / 2).toarray()) and np.array_equal(Mz, Mz.conj().T)
    assert "not checked" in utils.spai.__doc__.replace("NOT", "not")


def test_inputs_and_widening(spai_double):
    """A SciPy matrix of any format, a dense array and a MatrixLinearOperator give the same matrix; duplicates are summed, stored
    zeros stay in the pattern; fp32 is widened to fp64, complex64 to complex128."""
    from krypy_amd import utils

    A = sc.convection_x(6, 5)
    ref = utils.spai(A)
    for B in (A.tocsc(), A.tocoo(), A.toarray(), utils.MatrixLinearOperator(A)):
        _same_matrix(utils.spai(B), ref)
    C = A.tocoo()
    dup = sp.coo_matrix((np.concatenate([C.data[::-1] * 0.5, C.data[::-1] * 0.5]), (np.concatenate([C.row[::-1]] * 2),
                                                                                  np.concatenate([C.col[::-1]] * 2))), shape=A.shape)
    _same_matrix(utils.spai(dup), ref)
    # a stored zero stays in the pattern of A and so in the default pattern of M
    Z = sp.csr_matrix(A + sp.csr_matrix(([1.0], ([7], [1])), shape=A.shape))
    Z.sort_indices()
    Z.data[(Z.indices == 1) & (np.repeat(np.arange(30), np.diff(Z.indptr)) == 7)] = 0.0
    Mz = utils.spai(Z)
    assert Mz.nnz == A.nnz + 1 and 1 in Mz.indices[Mz.indptr[7]: Mz.indptr[8]]
    f32 = utils.spai(A.astype(np.float32))
    assert f32.dtype == np.float64
    _same_matrix(f32, utils.spai(A.astype(np.float32).astype(np.float64)))
    assert utils.spai(A.astype(np.complex64)).dtype == np.complex128
    assert utils.spai_operator(A.astype(np.float32)).dtype == np.float64


def test_argument_errors_never_reach_the_device(spai_double):
    from krypy_amd import utils

    A = sc.convection_x(7, 5)
    with pytest.raises(utils.ArgumentError):
        utils.spai(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(utils.ArgumentError):
        utils.spai(np.ones(4))
    with pytest.raises(utils.ArgumentError) as e:
        utils.spai(A, pattern=sp.identity(34, format="csr"))
    assert "shape" in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.spai(A, pattern=np.ones((35, 34)))
    with pytest.raises(utils.ArgumentError) as e:
        utils.spai(A, side="both")
    assert "side" in str(e.value)
    P = A.tolil()
    P[11, :33] = 1.0
    with pytest.raises(utils.ArgumentError) as e:
        utils.spai(A, pattern=P)
    assert "row 11" in str(e.value) and "33" in str(e.value) and "32" in str(e.value)
    with pytest.raises(utils.ArgumentError) as e:
        utils.spai(A, pattern=P.T, side="right")
    assert "column 11" in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.spai_operator(A, side="up")
    assert spai_double.calls.get("spai", 0) == 0          # all refused before anything reaches the device
    P[11, 32] = 0.0          # 32 entries are fine
    assert utils.spai(A, pattern=P.tocsr()).info["qmax"] == 32
    assert utils.spai(A, pattern=P.tocsr()).info["group_width"] == 32


def test_breakdown_is_an_argument_error(spai_double):
    from krypy_amd import utils

    for name, row in (("identical_rows", 3), ("zero_row", 8), ("two_broken_rows", 3)):
        A, P, _, _ = sc.oracle(name)
        with pytest.raises(utils.ArgumentError) as e:
            utils.spai(A, pattern=P)
        assert "SPAI breaks down: rows of A selected by pattern row %d are linearly dependent" % row in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.spai_operator(sc.oracle("zero_row")[0])
