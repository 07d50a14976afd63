"""GPU tests of the factorized sparse approximate inverse on a fixed lower-triangular pattern (krypy_amd/csrc/fsai.hip): u and d
must be the oracle's sequential loop (tests/support/fsai_ref.py) bit for bit, and a solver preconditioned with
``utils.fsai_operator`` must produce the bits of the same solver given ``MatrixLinearOperator`` of the oracle's matrix."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import fsai_cases as fc
from tests.support.fsai_numpy_context import launch_figures
from tests.support.fsai_ref import scaled
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
needs_single = pytest.mark.skipif(FORCED, reason="KRYPY_AMD_TEST_FORCE_MULTI=1: the context has a communicator, kh_fsai_build "
                                                 "refuses (test_refused_on_a_context_with_a_communicator holds that)")

BIT_CASES = (["band_%d" % n for n in (1, 2, 3, 63, 64, 65, 257)] + ["zband_%d" % n for n in (1, 2, 3, 63, 64, 65, 257)]
             + ["lap_A%d" % k for k in (1, 2, 3, 4)] + ["zlap_A%d" % k for k in (1, 2, 3, 4)]
             + ["random_20001", "zrandom_20001", "long_row", "zlong_row", "q1", "zq1", "diagonal", "zdiagonal"])


def _check_info(info, A, P, cplx, bad=-1):
    """The launch figures for WHATEVER width the library chose (no test depends on the measured choice)."""
    n, qmax = A.shape[0], int(np.diff(P.indptr).max())
    assert (info["n"], info["pnnz"], info["qmax"], info["first_broken_row"]) == (n, P.nnz, qmax, bad), info
    assert info["group_width"] in (8, 16, 32, 64), info
    wgs, lds = launch_figures(n, qmax, cplx, info["group_width"])
    expect_kernel((info["workgroups"], info["lds_bytes"]) == (wgs, lds), "launch figures %r, expected %r" % (info, (wgs, lds)))
    assert 0 < info["lds_bytes"] <= 65536


@needs_single
@pytest.mark.parametrize("name", BIT_CASES)
def test_bits_of_the_oracle(hip, name):
    """Banded matrices with sizes around one workgroup's rows (n = 1 .. 257: rows of q = 1 .. 4, an n that is no multiple of the
    rows per workgroup), the 37 x 23 grid with tril(A), tril(A^2), tril(A^3), tril(A^4) (q = 3, 7, 13, 21: every width the rule
    may choose from), 20001 rows of a random symmetric pattern, one row of exactly 32 pattern entries among rows of 1 and 2 (the
    loops run to 32 with most rows predicated off early), and patterns with q = 1 in every row."""
    A, P, U, d, bad = fc.oracle(name)
    assert bad == -1
    cplx = A.dtype.kind == "c"
    b0 = hip.get("n_fsai_build")
    u, dd, info = hip.fsai(A, P)
    bits_equal(u, U.data, name + " u")
    bits_equal(dd, d, name + " d")
    _check_info(info, A, P, cplx)
    assert hip.get("n_fsai_build") - b0 == 1 and hip.get("fsai_device_us") > 0
    q = np.diff(P.indptr)
    if name.endswith("long_row"):
        assert q.max() == 32 and np.sort(q)[-2] == 2
    if name.endswith("q1") or name.endswith("diagonal"):
        assert q.max() == 1 and np.all(u == 1.0)
    if "lap_A" in name:
        assert q.max() == {1: 3, 2: 7, 3: 13, 4: 21}[int(name[-1])]
    if name.endswith("20001"):
        assert q.min() == 1 and q.max() >= 4 and A.shape[0] % 32 != 0


@needs_single
@pytest.mark.parametrize("name", ["lap_A3", "zlap_A3"])
def test_twenty_repeats_give_identical_bits(hip, name):
    A, P, U, d, _ = fc.oracle(name)
    b0 = hip.get("n_fsai_build")
    for _ in range(20):
        u, dd, _info = hip.fsai(A, P)
        bits_equal(u, U.data, "repeat u")
        bits_equal(dd, d, "repeat d")
    assert hip.get("n_fsai_build") - b0 == 20


@needs_single
@pytest.mark.parametrize("name,row", [("missing_diagonal", 5), ("zmissing_diagonal", 5), ("indefinite", 1), ("zindefinite", 1),
                                      ("indefinite_A2", 1)])
def test_breakdown_is_reported_not_raised(hip, name, row):
    """The C call returns 0, names the smallest broken row and hands back what IEEE arithmetic made of it - the oracle's bits,
    the non-finite ones included; utils.fsai turns it into an ArgumentError."""
    from krypy_amd import utils

    A, P, U, d, bad = fc.oracle(name)
    assert bad == row
    u, dd, info = hip.fsai(A, P)
    nf = ~np.isfinite(U.data.view(np.float64))
    print("%s: %d non-finite words; device %s\n%s: oracle %s" % (name, nf.sum(), [hex(v) for v in u.view(np.uint64)[nf][:14]], name,
                                                                  [hex(v) for v in U.data.view(np.uint64)[nf][:14]]))
    assert info["first_broken_row"] == row
    if name == "indefinite_A2":          # d_1 = 0 exactly in the middle of row 2: L_21 = -1 / 0, and NaN follows
        assert nf.any() and np.isnan(d[2]) and np.isnan(dd[2])
    bits_equal(u, U.data, name + " u")
    bits_equal(dd, d, name + " d")
    _check_info(info, A, P, A.dtype.kind == "c", bad=row)
    with pytest.raises(utils.ArgumentError) as e:
        utils.fsai(A, pattern=P)
    assert "A is not positive definite: the principal submatrix selected by pattern row %d" % row in str(e.value)


def _raw_csr(n, indptr, indices, data=None):
    M = sp.csr_matrix((n, n))
    M.indptr, M.indices = np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32)
    M.data = np.ones(len(indices)) if data is None else np.asarray(data, dtype=float)
    return M


@needs_single
def test_argument_errors(hip):
    from krypy_amd import _hip, utils

    b0 = hip.get("n_fsai_build")
    good = _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 0, 1, 2], [4.0, 1.0, 4.0, 1.0, 1.0, 4.0])

    def refused(word, A, P):
        with pytest.raises(_hip.BackendError) as e:
            hip.fsai(A, P)
        assert "status -2" in str(e.value) and word in str(e.value), str(e.value)

    unsorted = _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 1, 0, 2])
    refused("unsorted column indices in row 2 of A", unsorted, good)
    refused("unsorted column indices in row 2 of the pattern", good, unsorted)
    refused("duplicate column indices in row 2 of the pattern", good, _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 0, 0, 2]))
    refused("duplicate column indices in row 2 of A", _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 0, 0, 2]), good)
    refused("column 7 out of range in row 2 of A", _raw_csr(3, [0, 1, 3, 5], [0, 0, 1, 0, 7]), good)
    refused("column 7 out of range in row 2 of the pattern", good, _raw_csr(3, [0, 1, 3, 5], [0, 0, 1, 0, 7]))
    refused("pattern row 1 is empty", good, _raw_csr(3, [0, 1, 1, 2], [0, 2]))
    refused("pattern row 1 ends in column 0", good, _raw_csr(3, [0, 1, 2, 3], [0, 0, 2]))
    refused("pattern row 0 ends in column 1", good, _raw_csr(3, [0, 2, 3, 4], [0, 1, 1, 2]))
    A = fc.band(40, 17, 3)
    P = sp.csr_matrix(sp.identity(40)).tolil()
    P[35, 3:35] = 1.0          # 32 below the diagonal and the diagonal
    refused("pattern row 35 has 33 entries, at most 32", A, sp.csr_matrix(P))
    with pytest.raises(_hip.BackendError):
        hip.fsai(sp.csr_matrix(np.ones((3, 4))), sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(_hip.BackendError):
        hip.fsai(good, sp.csr_matrix(np.tril(np.ones((4, 4)))))
    with pytest.raises(utils.ArgumentError) as e:
        utils.fsai(A, pattern=P)
    assert "row 35" in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.fsai((sp.tril(A) + 2.0 * sp.triu(A, 1)).tocsr())          # not Hermitian
    with pytest.raises(utils.ArgumentError):
        utils.fsai_operator(A, form="dense")
    assert hip.get("n_fsai_build") == b0          # error returns, nothing ran


def test_refused_on_a_context_with_a_communicator():
    """Sharded construction does not exist: a context in multi-rank mode refuses and says why."""
    from krypy_amd import _hip

    os.environ["KRYPY_AMD_FORCE_MULTI"] = "1"
    try:
        ctx = _hip.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
    finally:
        del os.environ["KRYPY_AMD_FORCE_MULTI"]
    try:
        A = fc.grid(False, 4, 3)
        with pytest.raises(_hip.BackendError) as e:
            ctx.fsai(A, sp.tril(A).tocsr())
        assert "status -5" in str(e.value) and "communicator" in str(e.value)
    finally:
        ctx.close()


# ---- solvers ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _system(cplx):
    """(A, b) on the 37 x 23 grid - computed once, shared."""
    A = fc.grid(cplx)
    rng = np.random.default_rng(0)
    b = rng.standard_normal((A.shape[0], 1))
    if cplx:
        b = b + 1j * rng.standard_normal((A.shape[0], 1))
    return A, b


@functools.lru_cache(maxsize=None)
def _oracle_matrices(cplx, k):
    """(G, G^H, G^H G) of the oracle for the pattern tril(A^k), as utils.fsai_operator forms them."""
    A, P, U, d, bad = fc.oracle("%slap_A%d" % ("z" if cplx else "", k))
    assert bad == -1
    G = scaled(U, d)
    Gh = G.conj().T.tocsr()
    Gh.sort_indices()
    M = (Gh @ G).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    return G, Gh, M


def _run(solver, A, b, maxiter, tol, **kw):
    from krypy_amd import linsys, utils

    ls = linsys.LinearSystem(A, b, **kw)
    try:
        sol = solver(ls, tol=tol, maxiter=maxiter)
        return np.array(sol.resnorms), np.array(sol.xk), True
    except utils.ConvergenceError as e:
        return np.array(e.solver.resnorms), np.array(e.solver.xk), False


SPD = dict(self_adjoint=True, positive_definite=True)


@needs_single
@pytest.mark.parametrize("solver", ["Cg", "Minres"])
@pytest.mark.parametrize("cplx", [False, True])
def test_cg_minres_with_the_matrix_form_have_the_bits_of_the_oracles_matrix(hip, solver, cplx):
    """M = fsai_operator(A, form="matrix") built on the device against MatrixLinearOperator of G^H G formed from the oracle's G:
    the same matrix bit for bit, so the same residual norms and iterate bit for bit.  Complex: CG / MINRES on the Hermitian case."""
    from krypy_amd import linsys, utils

    A, b = _system(cplx)
    _, _, M = _oracle_matrices(cplx, 2)
    b0 = hip.get("n_fsai_build")
    op = utils.fsai_operator(A, pattern=A @ A, form="matrix")
    assert hip.get("n_fsai_build") - b0 == 1
    bits_equal(op._A.data, M.data, "G^H G")
    assert np.array_equal(op._A.indices, M.indices) and np.array_equal(op._A.indptr, M.indptr)
    S = getattr(linsys, solver)
    res_d, x_d, ok = _run(S, A, b, 200, 1e-8, M=op, **SPD)
    res_t, x_t, ok_t = _run(S, A, b, 200, 1e-8, M=utils.MatrixLinearOperator(M), **SPD)
    assert ok and ok_t
    bits_equal(res_d, res_t, "resnorms")
    bits_equal(x_d, x_t, "xk")
    r = np.linalg.norm(b - A @ x_d) / np.linalg.norm(b)
    assert r <= 1e-6, r          # (the solver's tolerance is on the preconditioned residual)
    print("%s %s: %d iterations" % (solver, "c128" if cplx else "fp64", len(res_d) - 1))


class _Spy(object):
    """Records calls of the named methods of a context (the first argument after the operator handle that matters to the test:
    the kind of Md for the fused steps, nothing for apply)."""

    def __init__(self, ctx, names, pick):
        self.ctx, self.names, self.pick, self.seen = ctx, names, pick, []

    def __enter__(self):
        for name in self.names:
            real = getattr(self.ctx, name)

            def spy(*a, _real=real, **kw):
                self.seen.append(self.pick(a))
                return _real(*a, **kw)

            setattr(self.ctx, name, spy)
        return self

    def __exit__(self, *exc):
        for name in self.names:
            delattr(self.ctx, name)


@needs_single
def test_the_matrix_form_rides_the_fused_arnoldi_step(hip):
    """M = fsai_operator(A, form="matrix") in GMRES on the self-adjoint system: every call that asks for fused Arnoldi steps hands
    the CSR matrix over as Md, and "n_cycle_steps", which only the fused steps inside kh_gmres_cycle raise, grows by the
    iterations - the external-operator path would leave both empty.  Bits of the oracle's matrix."""
    from krypy_amd import linsys, utils

    A, b = _system(False)
    _, _, M = _oracle_matrices(False, 2)
    op = utils.fsai_operator(A, pattern=A @ A, form="matrix")
    c0 = hip.get("n_cycle_steps")
    with _Spy(hip, ("arnoldi_step", "arnoldi_step_begin", "gmres_cycle"), lambda a: None if a[1] is None else a[1].kind) as spy:
        res, x, ok = _run(linsys.Gmres, A, b, 120, 1e-8, M=op, **SPD)
    steps = hip.get("n_cycle_steps") - c0
    assert ok
    expect_kernel(len(spy.seen) >= 1 and set(spy.seen) == {"csr"}, "calls for fused steps with a matrix Md: kinds %r" % (spy.seen[:8],))
    expect_kernel(steps >= len(res) - 2, "n_cycle_steps grew by %d in %d iterations" % (steps, len(res) - 1))
    res_t, x_t, _ = _run(linsys.Gmres, A, b, 120, 1e-8, M=utils.MatrixLinearOperator(M), **SPD)
    bits_equal(res, res_t, "resnorms")
    bits_equal(x, x_t, "xk")


@needs_single
@pytest.mark.parametrize("cplx", [False, True])
def test_the_factored_form_is_two_applies_and_agrees_with_the_matrix_form(hip, cplx):
    """form="factored": one application on device blocks is exactly two kh_apply (G, then G^H) and no upload or download; CG with
    it converges like CG with the matrix form - the same iteration count within one, the iterates equal to the solver tolerance
    (1e-8 on the relative residual, times cond(A) <= 334 for the error)."""
    from krypy_amd import linsys, utils

    A, b = _system(cplx)
    G, Gh, M = _oracle_matrices(cplx, 2)
    fac = utils.fsai_operator(A, pattern=A @ A)
    bits_equal(fac.args[1]._A.data, G.data, "G")
    bits_equal(fac.args[0]._A.data, Gh.data, "G^H")
    X = hip.upload(b)
    Y = hip.alloc(A.shape[0], 1, dtype=b.dtype)
    fac._apply_dev(X, 0, Y, 0, 1)          # (uploads the two matrices once)
    with _Spy(hip, ("apply", "upload", "alloc"), lambda a: None) as spy:
        fac._apply_dev(X, 0, Y, 0, 1)
    assert len(spy.seen) == 2, "one application made %d calls of apply / upload / alloc, two kh_apply expected" % len(spy.seen)
    y0 = Gh @ (G @ b)
    assert np.abs(Y.download() - y0).max() <= 64 * np.finfo(float).eps * np.abs(y0).max()
    res_f, x_f, ok_f = _run(linsys.Cg, A, b, 200, 1e-8, M=fac, **SPD)
    res_m, x_m, ok_m = _run(linsys.Cg, A, b, 200, 1e-8, M=utils.fsai_operator(A, pattern=A @ A, form="matrix"), **SPD)
    assert ok_f and ok_m and abs(len(res_f) - len(res_m)) <= 1, (len(res_f), len(res_m))
    assert np.linalg.norm(x_f - x_m) <= 1e-8 * 334 * np.linalg.norm(x_m) * 4


@needs_single
def test_gmres_split_with_the_factor_and_its_adjoint(hip):
    """GMRES with Ml = G, Mr = G^H (the split form: G A G^H y = G b, x = G^H y) converges in fewer iterations than plain GMRES and
    has the bits of the same solve given the oracle's factors."""
    from krypy_amd import linsys, utils

    A, b = _system(False)
    G, Gh, _ = _oracle_matrices(False, 2)
    Gd = utils.fsai(A, A @ A)
    bits_equal(Gd.data, G.data, "G")
    Ghd = Gd.conj().T.tocsr()
    Ghd.sort_indices()
    res, x, ok = _run(linsys.Gmres, A, b, 120, 1e-8, Ml=utils.MatrixLinearOperator(Gd), Mr=utils.MatrixLinearOperator(Ghd))
    res_t, x_t, _ = _run(linsys.Gmres, A, b, 120, 1e-8, Ml=utils.MatrixLinearOperator(G), Mr=utils.MatrixLinearOperator(Gh))
    assert ok
    bits_equal(res, res_t, "resnorms")
    bits_equal(x, x_t, "xk")
    res_0, _, ok_0 = _run(linsys.Gmres, A, b, len(res) - 1, 1e-8)
    assert not ok_0, "plain GMRES needs no more than the preconditioned one's %d iterations" % (len(res) - 1)
    assert np.linalg.norm(b - A @ x) <= 1e-6 * np.linalg.norm(b)


@needs_single
def test_iteration_counts_fall_with_the_pattern(hip):
    """CG to 1e-8 on the 37 x 23 grid: its(tril A^4) < its(tril A^2) < its(tril A) < its(plain).  SciPy's CG counts 25 < 40 < 56
    < 106 there - wide margins; the project's own counts are what is compared."""
    from krypy_amd import linsys, utils

    A, b = _system(False)
    its = []
    for k in (None, 1, 2, 4):
        kw = dict(SPD)
        if k is not None:
            kw["M"] = utils.fsai_operator(A, pattern=fc.power_pattern(A, k), form="matrix")
        res, _, ok = _run(linsys.Cg, A, b, 400, 1e-8, **kw)
        assert ok
        its.append(len(res) - 1)
    print("CG iterations, plain / tril(A) / tril(A^2) / tril(A^4):", its)
    assert its[3] < its[2] < its[1] < its[0], its
