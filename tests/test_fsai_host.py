"""CPU tests of the factorized sparse approximate inverse on a fixed lower-triangular pattern: the oracle
(tests/support/fsai_ref.py) against independent facts, krypy_amd/csrc/fsai.h as a stand-alone sanitizer build, and the host layer
(``utils.fsai``, ``utils.fsai_operator``) on a NumPy context whose ``fsai`` is the oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import fsai_cases as fc
from tests.support.fsai_ref import fsai_matrix, fsai_ref, lower_pattern, scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


@pytest.fixture
def fsai_double():
    from krypy_amd import _hip
    from tests.support.fsai_numpy_context import FsaiNumpyContext

    ctx = FsaiNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


def _G(name):
    A, P, U, d, bad = fc.oracle(name)
    assert bad == -1
    return A, P, scaled(U, d)


def _cond_preconditioned(A, G):
    return np.linalg.cond((G @ A @ G.conj().T).toarray())


# ---- the oracle against independent facts ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lap_A1", "lap_A2", "lap_A3", "zlap_A1", "zlap_A2", "band_65", "zband_65", "long_row", "zlong_row"])
def test_oracle_rows_satisfy_the_defining_equations(name):
    """For every row i with pattern columns J: (G A)[i, J_b] = 0 for b < q - 1 and (G A G^H)_ii = 1, against dense NumPy products,
    and the row equals y / sqrt(y_last) with y = numpy.linalg.solve(A[J, J]^T, e_last) (an LU factorisation with pivoting, not the
    oracle's LDL^H route; the ROW g solves g A[J, J] = e_last^T / g_last, so it is the TRANSPOSED submatrix that is solved with:
    for real data that is A[J, J] itself, for Hermitian data y is the conjugate of numpy.linalg.solve(A[J, J], e_last)).
    Bar: 64 eps cond(A[J, J]), relative to the row's largest entry for the solution, absolute for the residuals of the scaled
    equations (G A G^H has a unit diagonal) - the bar of test_spai_host.py for its rows."""
    A, P, G = _G(name)
    D = A.toarray()
    Gd = G.toarray()
    GA = Gd @ D
    GAG = GA @ Gd.conj().T
    worst = 0.0
    for i in range(A.shape[0]):
        J = P.indices[P.indptr[i]: P.indptr[i + 1]]
        assert J[-1] == i
        sub = D[np.ix_(J, J)]
        bar = 64 * EPS * np.linalg.cond(sub)
        scale = np.abs(D[i, i]) ** 0.5          # (G A)[i, :] carries the scale of sqrt(A_ii)
        r0 = np.abs(GA[i, J[:-1]]).max() / scale if J.size > 1 else 0.0
        r1 = abs(GAG[i, i] - 1.0)
        e = np.zeros(J.size, dtype=D.dtype)
        e[-1] = 1.0
        y = np.linalg.solve(sub.T, e)
        assert np.allclose(y, np.linalg.solve(sub, e).conj(), rtol=0, atol=bar * np.abs(y).max())
        assert abs(y[-1].imag) <= bar * abs(y[-1]) and y[-1].real > 0
        want = y / np.sqrt(y[-1].real)
        got = G.data[P.indptr[i]: P.indptr[i + 1]]
        err = np.abs(got - want).max() / np.abs(want).max()
        worst = max(worst, max(r0, r1, err) / bar)
        assert r0 <= bar and r1 <= bar and err <= bar, (i, r0, r1, err, bar)
    assert 0 <= worst <= 1
    assert sp.triu(G, 1).nnz == 0


@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_is_the_inverse_cholesky_factor_on_the_full_lower_pattern(cplx):
    """A dense SPD / Hermitian positive definite matrix of n = 24 with the full lower-triangular pattern: G = inv(cholesky(A))
    (measured: max error 1.4e-17 / 1.7e-17 in the prototype).  Bar: 64 eps cond(A) relative to the largest entry."""
    rng = np.random.default_rng(7)
    B = rng.standard_normal((24, 24)) + (1j * rng.standard_normal((24, 24)) if cplx else 0.0)
    A = B @ B.conj().T + 24.0 * np.eye(24)
    G = fsai_matrix(sp.csr_matrix(A), np.ones((24, 24))).toarray()
    want = np.linalg.inv(np.linalg.cholesky(A))
    err = np.abs(G - want).max() / np.abs(want).max()
    assert err <= 64 * EPS * np.linalg.cond(A), err
    assert np.abs(G @ A @ G.conj().T - np.eye(24)).max() <= 64 * EPS * np.linalg.cond(A)


# ---- quality -------------------------------------------------------------------------------------------------------------
def test_quality_on_the_grid_real():
    """37 x 23 five-point Laplacian, cond(A) = 333.2: cond(G A G^H) for the patterns tril(A), tril(A^2), tril(A^3), tril(A^4) is
    strictly decreasing and below cond(A) - the oracle's figures: 93.8 / 47.2 / 28.1 / 18.6 (a prototype had 28.0 / 18.5) - and
    G^H G has only positive eigenvalues."""
    A = fc.grid()
    conds = [np.linalg.cond(A.toarray())]
    for k in (1, 2, 3, 4):
        _, _, G = _G("lap_A%d" % k)
        conds.append(_cond_preconditioned(A, G))
        M = (G.conj().T @ G).toarray()
        assert np.array_equal(M, M.T) or np.allclose(M, M.T, rtol=0, atol=4 * EPS * np.abs(M).max())
        assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0
    print("cond(A), cond(G A G^H) for tril(A^k), k = 1..4:", ["%.1f" % c for c in conds])
    assert conds[0] > conds[1] > conds[2] > conds[3] > conds[4] > 1
    assert np.allclose(conds, [333.2, 93.8, 47.2, 28.1, 18.6], rtol=0, atol=0.06)


def test_quality_on_the_grid_hermitian():
    """A + 0.5 I + 0.3i (K - K^T), K = triu(A, 1): Hermitian, positive definite by diagonal dominance, cond = 24.8; cond(G A G^H)
    falls to 7.4 with tril(A) and to 4.0 with tril(A^2)."""
    A = fc.grid(True)
    assert (A != A.conj().T).nnz == 0 and np.iscomplexobj(A.data) and np.abs(A.data.imag).max() == 0.3
    conds = [np.linalg.cond(A.toarray())]
    for k in (1, 2):
        _, _, G = _G("zlap_A%d" % k)
        assert np.iscomplexobj(G.data)
        conds.append(_cond_preconditioned(A, G))
        M = (G.conj().T @ G).toarray()
        assert np.linalg.eigvalsh((M + M.conj().T) / 2).min() > 0
    print("Hermitian case: cond(A), cond(G A G^H) for tril(A), tril(A^2):", ["%.1f" % c for c in conds])
    assert conds[0] > conds[1] > conds[2] > 1
    assert np.allclose(conds, [24.8, 7.4, 4.0], rtol=0, atol=0.06)


# ---- exact cases and breakdowns that are exact by construction ---------------------------------------------------------------
def test_oracle_exact_cases():
    dvals = np.linspace(0.5, 4.0, 9)
    for name in ("diagonal", "zdiagonal"):
        A, P, U, d, bad = fc.oracle(name)
        assert bad == -1 and U.nnz == 9 and np.array_equal(U.data, np.ones(9)) and np.array_equal(d, dvals)
        assert np.array_equal(scaled(U, d).diagonal(), 1.0 / np.sqrt(dvals))
    U, d, bad = fsai_ref(sp.csr_matrix(np.array([[2.5]])))          # n = 1
    assert bad == -1 and U.toarray() == [[1.0]] and d[0] == 2.5
    A, P, U, d, bad = fc.oracle("q1")          # the pattern of the identity on a grid matrix: q = 1 everywhere
    assert bad == -1 and np.array_equal(U.data, np.ones(63)) and np.array_equal(d, A.diagonal())
    # a 2 x 2 matrix in small integers: L = 1/2, d = (4, 3): u = (-1/2, 1), all exact
    U, d, bad = fsai_ref(sp.csr_matrix(np.array([[4.0, 2.0], [2.0, 4.0]])))
    assert bad == -1 and np.array_equal(U.toarray(), [[1.0, 0.0], [-0.5, 1.0]]) and np.array_equal(d, [4.0, 3.0])
    # the complex back substitution takes L unconjugated: A = [[4, 2 - 2i], [2 + 2i, 4]], L_10 = (2 + 2i) / 4, u_0 = -L_10
    U, d, bad = fsai_ref(sp.csr_matrix(np.array([[4.0, 2.0 - 2.0j], [2.0 + 2.0j, 4.0]])))
    assert bad == -1 and U[1, 0] == -0.5 - 0.5j and np.array_equal(d, [4.0, 2.0])
    G = scaled(U, d).toarray()
    assert np.abs(G @ np.array([[4.0, 2.0 - 2.0j], [2.0 + 2.0j, 4.0]]) @ G.conj().T - np.eye(2)).max() <= 4 * EPS


def test_oracle_breakdowns():
    """Exact by construction.  The missing stored diagonal (5, 5): S_jj = +0, the pivot is minus a sum of |L|^2 d over positive
    d - row 5 is the first.  A - 3 I on the grid is indefinite: row 0 has d = 1, row 1 has d = 1 - (-1 / 1) * (-1) = 0 exactly
    (small integers) - the oracle breaks first in row 1, as the prototype did.  The loop goes on: rows that do not touch the broken
    pivot stay finite."""
    for name in ("missing_diagonal", "zmissing_diagonal"):
        A, P, U, d, bad = fc.oracle(name)
        assert bad == 5 and d[5] <= 0 and np.all(d[:5] > 0)
        assert np.all(np.isfinite(U.data[: P.indptr[5]])) and np.all(d[8:] > 0)
    A, P, U, d, bad = fc.oracle("indefinite")
    assert bad == 1 and d[0] == 1.0 and d[1] == 0.0
    assert np.linalg.eigvalsh(A.toarray()).min() < 0
    A, P, U, d, bad = fc.oracle("zindefinite")
    assert bad == 1 and d[0] == 1.0 and d[1] < 0
    A, P, U, d, bad = fc.oracle("indefinite_A2")          # the zero pivot in the middle of row 2: -inf and NaN follow
    assert bad == 1 and list(P.indices[P.indptr[2]: P.indptr[3]]) == [0, 1, 2] and np.isnan(d[2])
    assert d[2:3].view(np.uint64)[0] == 0x7ff8000000000000 and not np.all(np.isfinite(U.data[P.indptr[2]: P.indptr[3]]))


def test_only_the_lower_triangle_is_read():
    A = fc.band(20, 3, 4)
    B = (sp.tril(A) + 7.0 * sp.triu(fc.band(20, 3, 9), 1)).tocsr()
    assert (B != B.T).nnz > 0
    U, d, bad = fsai_ref(A)
    U2, d2, bad2 = fsai_ref(B, lower_pattern(A))
    assert bad == bad2 == -1 and np.array_equal(U.data, U2.data) and np.array_equal(d, d2)


# ---- krypy_amd/csrc/fsai.h alone, under the host sanitizers ----------------------------------------------------------------
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
    """krypy_amd/csrc/fsai.h is plain C++: compiled alone into a program with its own main (tests/support/fsai_main.cpp) with
    -fsanitize=address,undefined and run on the CPU as a child process.  For every case, real and complex, the program computes
    all rows with a plain sequential loop of its own and with the header's row routine on 1 / 8 / 16 / 32 / 64 emulated lanes -
    the split the kernel makes - and compares the bits of u and d; then it feeds the validation every kind of bad input."""
    exe = str(tmp_path / "fsai_main")
    subprocess.check_call(_compiler() + ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "krypy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "support", "fsai_main.cpp"), "-o", exe])
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
    want_q = {"grid_tril_A": 3, "grid_tril_A2": 7, "grid_tril_A3": 13, "grid_tril_A4": 21, "band_q32": 32, "diagonal": 1, "n1": 1,
              "missing_diagonal": 3, "indefinite": 3}
    want_bad = {"missing_diagonal": 5, "indefinite": 1}
    for case, q in want_q.items():
        for kind in "rz":
            for W in (1, 8, 16, 32, 64):
                g = runs["%s/%s/%d" % (case, kind, W)]
                assert g["bits"] == "ok" and int(g["q"]) == q, (case, kind, W, g)
                assert int(g["bad"]) == want_bad.get(case, -1), (case, kind, W, g)
    assert len(runs) == len(want_q) * 2 * 5
    for name, word in (("n_zero", "n = 0 out of range"), ("n_too_large", "n = 2147483648 out of range"),
                       ("nnz_too_large", "nnz = 2147483648 of A out of range"),
                       ("unsorted_A", "unsorted column indices in row 5 of A"),
                       ("unsorted_pattern", "unsorted column indices in row 15 of the pattern"),
                       ("duplicate_A", "duplicate column indices in row 6 of A"),
                       ("duplicate_pattern", "duplicate column indices in row 16 of the pattern"),
                       ("out_of_range_A", "column 117 out of range in row 7 of A"),
                       ("out_of_range_pattern", "column 117 out of range in row 7 of the pattern"),
                       ("negative_column", "column -1 out of range in row 2 of A"),
                       ("indptr_not_ascending", "not ascending at row 2"),
                       ("upper_entries", "pattern row 0 ends in column 9"),
                       ("empty_row", "pattern row 7 is empty"),
                       ("no_diagonal", "pattern row 11 ends in column 10"),
                       ("q33", "pattern row 32 has 33 entries, at most 32")):
        assert word in refused[name], (name, refused.get(name))
    assert len(refused) == 15


# ---- the Python layer on the NumPy context -------------------------------------------------------------------------------
def _same_matrix(got, want):
    got = sp.csr_matrix(got)
    assert got.has_sorted_indices and got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64))


@pytest.mark.parametrize("name", ["lap_A1", "lap_A2", "zlap_A2"])
def test_fsai_and_both_forms_of_the_operator(fsai_double, name):
    from krypy_amd import utils
    from tests.support.fsai_numpy_context import launch_figures

    A, P, want = _G(name)
    k = int(name[-1])
    given = None if k == 1 else A @ A
    G = utils.fsai(A, given)
    _same_matrix(G, want)
    assert sp.triu(G, 1).nnz == 0
    info = G.info
    qmax = int(np.diff(P.indptr).max())
    assert (info["n"], info["pnnz"], info["qmax"], info["first_broken_row"]) == (A.shape[0], P.nnz, qmax, -1)
    assert qmax == {1: 3, 2: 7}[k]
    assert info["group_width"] in (8, 16, 32, 64)
    assert (info["workgroups"], info["lds_bytes"]) == launch_figures(A.shape[0], qmax, A.dtype.kind == "c", info["group_width"])
    assert sorted(info) == ["first_broken_row", "group_width", "lds_bytes", "n", "pnnz", "qmax", "workgroups"]
    # the pattern as a dense array, as a sparse matrix of another format, with other values, or already lower: only tril is read
    for Pm in ((A @ A).toarray(), (A @ A).tocoo(), 7.0 * (A @ A), sp.tril(A @ A)) if k == 2 else (A, sp.tril(A), sp.tril(A, -1)):
        _same_matrix(utils.fsai(A, Pm), want)
    Gh = want.conj().T.tocsr()
    Gh.sort_indices()
    x = np.random.default_rng(1).standard_normal((A.shape[0], 2)) + (1j if A.dtype.kind == "c" else 0)
    fac = utils.fsai_operator(A, pattern=given)
    assert isinstance(fac, utils._ProductLinearOperator) and fac.shape == A.shape and fac.dtype == A.dtype
    assert all(isinstance(a, utils.MatrixLinearOperator) for a in fac.args)
    _same_matrix(fac.args[0]._A, Gh)
    _same_matrix(fac.args[1]._A, want)
    _same_matrix(fac.G, want)
    mat = utils.fsai_operator(A, pattern=given, form="matrix")
    assert isinstance(mat, utils.MatrixLinearOperator) and mat.info == info
    M = (Gh @ want).tocsr()
    M.sort_indices()
    _same_matrix(mat._A, M)
    Md = mat._A.toarray()
    assert mat._A.nnz > want.nnz and np.allclose(Md, Md.conj().T, rtol=0, atol=4 * EPS * np.abs(Md).max())
    y0 = Gh @ (want @ x)
    assert np.allclose(fac.dot(x), y0, rtol=0, atol=64 * EPS * np.abs(y0).max())
    assert np.allclose(mat.dot(x), y0, rtol=0, atol=64 * EPS * np.abs(y0).max())
    # the fill trade-off the docstring states
    if name == "lap_A1":
        assert (want.nnz, M.nnz) == (2493, 5719)
    assert fsai_double.calls["fsai"] >= 5


def test_inputs_and_widening(fsai_double):
    from krypy_amd import utils

    A = fc.grid(False, 6, 5)
    ref = utils.fsai(A)
    for B in (A.tocsc(), A.tocoo(), A.toarray(), utils.MatrixLinearOperator(A)):
        _same_matrix(utils.fsai(B), ref)
    # a stored zero in the lower triangle stays in the pattern
    Z = sp.csr_matrix(A + sp.csr_matrix(([1.0, 1.0], ([7, 1], [1, 7])), shape=A.shape))
    Z.sort_indices()
    rows = np.repeat(np.arange(30), np.diff(Z.indptr))
    Z.data[((Z.indices == 1) & (rows == 7)) | ((Z.indices == 7) & (rows == 1))] = 0.0
    Gz = utils.fsai(Z)
    assert Gz.nnz == ref.nnz + 1 and 1 in Gz.indices[Gz.indptr[7]: Gz.indptr[8]]
    f32 = utils.fsai(A.astype(np.float32))
    assert f32.dtype == np.float64
    _same_matrix(f32, ref)
    assert utils.fsai(A.astype(np.complex64)).dtype == np.complex128
    assert utils.fsai_operator(A.astype(np.float32)).dtype == np.float64
    assert utils.fsai_operator(A.astype(np.float32), form="matrix").dtype == np.float64


def test_check_and_the_lower_triangle(fsai_double):
    """A non-Hermitian A: refused with check=True; with check=False the result is that of the Hermitian matrix with the same lower
    triangle - and the docstring says so."""
    from krypy_amd import utils

    A = fc.band(20, 3, 4)
    B = (sp.tril(A) + 7.0 * sp.triu(fc.band(20, 3, 9), 1)).tocsr()
    with pytest.raises(utils.ArgumentError) as e:
        utils.fsai(B)
    assert "not Hermitian" in str(e.value)
    assert fsai_double.calls.get("fsai", 0) == 0
    _same_matrix(utils.fsai(B, check=False), utils.fsai(A))
    Z = fc.band(20, 3, 4, True)
    with pytest.raises(utils.ArgumentError):
        utils.fsai((sp.tril(Z) + sp.tril(Z, -1).T).tocsr())          # complex SYMMETRIC: transposed, not conjugated
    with pytest.raises(utils.ArgumentError):
        utils.fsai_operator(B, form="matrix")
    _same_matrix(utils.fsai_operator(B, check=False).G, utils.fsai(A))
    assert "lower triangle" in " ".join(utils.fsai.__doc__.lower().split())


def test_argument_errors_never_reach_the_device(fsai_double):
    from krypy_amd import utils

    A = fc.grid(False, 7, 5)
    with pytest.raises(utils.ArgumentError):
        utils.fsai(sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(utils.ArgumentError):
        utils.fsai(np.ones(4))
    with pytest.raises(utils.ArgumentError) as e:
        utils.fsai(A, pattern=sp.identity(34, format="csr"))
    assert "shape" in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.fsai(A, pattern=np.ones((35, 34)))
    with pytest.raises(utils.ArgumentError) as e:
        utils.fsai_operator(A, form="dense")
    assert "form" in str(e.value)
    P = A.tolil()
    P[34, :33] = 1.0          # 33 entries below the diagonal of row 34, the diagonal makes 34
    P[33, :31] = 1.0          # columns 0 .. 30, the neighbour 32 and the diagonal: 33
    with pytest.raises(utils.ArgumentError) as e:
        utils.fsai(A, pattern=P)
    assert "row 33" in str(e.value) and "33 entries" in str(e.value) and "32" in str(e.value)
    assert fsai_double.calls.get("fsai", 0) == 0          # all refused before anything reaches the device
    P = A.tolil()
    P[33, :] = 1.0          # 35 entries in the row, 34 in its lower triangle
    P[33, :2] = 0.0          # ... 32 now
    assert utils.fsai(A, pattern=P.tocsr()).info["qmax"] == 32


def test_breakdown_is_an_argument_error(fsai_double):
    from krypy_amd import utils

    for name, row in (("missing_diagonal", 5), ("zmissing_diagonal", 5), ("indefinite", 1), ("zindefinite", 1)):
        A = fc.oracle(name)[0]
        with pytest.raises(utils.ArgumentError) as e:
            utils.fsai(A)
        assert "A is not positive definite: the principal submatrix selected by pattern row %d" % row in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.fsai_operator(fc.oracle("indefinite")[0], form="matrix")
