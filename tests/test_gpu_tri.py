"""GPU tests of the sparse triangular solves (krypy_amd/csrc/tri.hip): the device result must be the oracle's sequential
substitution (tests/support/tri_ref.py) bit for bit - for every launch plan -, and a solver preconditioned with the device
operators must produce the bits of the same solver with a host-callable twin of them."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.support import tri_cases as tc
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal, poison
from tests.support.tri_ref import levels_ref, tri_solve_ref

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
needs_single = pytest.mark.skipif(FORCED, reason="KRYPY_AMD_TEST_FORCE_MULTI=1: the context has a communicator, kh_tri_create "
                                                 "refuses (test_refused_on_a_context_with_a_communicator holds that)")
_default = {}


def _default_narrow(ctx):
    """The library's own default of tri_narrow_rows, read once before this module sets anything."""
    if id(ctx) not in _default:
        _default[id(ctx)] = ctx.get("tri_narrow_rows")
    return _default[id(ctx)]


def _tri(ctx, T, lower, unit, narrow=None, dtype=None):
    default = _default_narrow(ctx)
    ctx.set("tri_narrow_rows", default if narrow is None else narrow)
    try:
        return ctx.tri(T, lower, unit, dtype=dtype)
    finally:
        ctx.set("tri_narrow_rows", default)


def _solve(ctx, t, b):
    X = ctx.upload(b, dtype=t.dtype)
    Y = ctx.alloc(X.n, X.ncols, dtype=t.dtype)
    ctx.tri_solve(t, X, 0, Y, 0, X.ncols)
    return Y.download()


def _plan(counts, narrow):
    """(wide launches, narrow launches) of the levels with `counts` rows each."""
    wide = nar = 0
    run = False
    for c in counts:
        if c <= narrow:
            nar += 0 if run else 1
            run = True
        else:
            wide += 1
            run = False
    return wide, nar


def _rhs(n, cplx, seed=0, k=1):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, k))
    return b + 1j * rng.standard_normal((n, k)) if cplx else b


@needs_single
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 3001, 4099, 70001])
def test_bits_of_the_sequential_substitution(hip, n):
    """Lower and upper, unit and stored diagonal, real and complex at sizes around the slice (64) and workgroup (256)
    boundaries, odd sizes, and 70001 rows (more than one workgroup per level, 1094 slices in the widest)."""
    for lower in (True, False):
        Tr = tc.random_triangular(n, min(1.0, 8.0 / n), 100 + n, lower=lower)
        for cplx in (False, True):
            T = tc.make_complex(Tr, n) if cplx else Tr
            b = _rhs(n, cplx, n)
            for unit in (False, True):
                t = _tri(hip, T, lower, unit)
                got = _solve(hip, t, b)
                bits_equal(got, tri_solve_ref(T, b, lower, unit), "n=%d lower=%s cplx=%s unit=%s" % (n, lower, cplx, unit))
                info = t.info()
                _, cnt = levels_ref(T, lower)
                assert (info["n"], info["nnz"], info["levels"], info["widest_level"]) == (n, T.nnz, len(cnt), cnt.max())


STRUCTURES = {
    "diagonal": lambda: sp.diags(np.linspace(1.0, 3.0, 777)).tocsr(),
    "bidiagonal_3001": lambda: tc.bidiagonal(3001),
    "rows_without_offdiagonals": lambda: tc.long_row(1200, width=1),
    "random_3001": lambda: tc.random_triangular(3001, 0.004, 29),
    "random_1025": lambda: tc.random_triangular(1025, 0.02, 42),
    "long_row_500": lambda: tc.long_row(2000, width=500),
    "natural_100x90": lambda: tc.triangle(tc.lap2d(100, 90), True),
    "wide_levels": lambda: tc.triangle(tc.lap2d(150, 140, "redblack"), True),
}


@needs_single
@pytest.mark.parametrize("narrow", [0, 64, None])
@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_structures_under_every_launch_plan(hip, name, narrow):
    """Each structure with tri_narrow_rows = 0 (every level a launch of its own), 64 (the two kinds alternate where levels are
    wider and narrower than a slice) and the default: the same bits; kh_tri_info and the counters say which kinds ran."""
    T = STRUCTURES[name]()
    n = T.shape[0]
    _, cnt = levels_ref(T, True)
    for cplx in (False, True):
        Tc = tc.make_complex(T, 3) if cplx else T
        Tu = Tc.T.tocsr()
        Tu.sort_indices()
        b = _rhs(n, cplx, 17)
        for M, lower in ((Tc, True), (Tu, False)):
            t = _tri(hip, M, lower, False, narrow)
            w0, n0, s0 = hip.get("n_tri_wide"), hip.get("n_tri_narrow"), hip.get("n_tri_solve")
            got = _solve(hip, t, b)
            bits_equal(got, tri_solve_ref(M, b, lower), "%s lower=%s cplx=%s narrow=%s" % (name, lower, cplx, narrow))
            info = t.info()
            counts = levels_ref(M, lower)[1]
            wide, nar = _plan(counts, _default_narrow(hip) if narrow is None else narrow)
            expect_kernel((info["wide_launches"], info["narrow_launches"]) == (wide, nar),
                          "%s: plan %r, expected %r" % (name, info, (wide, nar)))
            expect_kernel((hip.get("n_tri_wide") - w0, hip.get("n_tri_narrow") - n0, hip.get("n_tri_solve") - s0) == (wide, nar, 1),
                          "%s: counters" % name)
            assert info["levels"] == len(counts) and info["longest_row"] == int(np.diff(M.indptr).max()) - 1
            assert info["slots"] >= M.nnz - n
    if name == "bidiagonal_3001":
        assert len(cnt) == 3001
    if name == "natural_100x90":          # anti-diagonals 1 .. 90 .. 1: with 64 a narrow run, the wide middle, a narrow run
        assert len(cnt) == 189 and cnt.max() == 90 and _plan(cnt, 64) == (189 - 2 * 64, 2)
    if name == "wide_levels":
        assert list(cnt) == [10500, 10500]
    if name == "long_row_500":
        assert int(np.diff(T.indptr).max()) >= 501


@needs_single
@pytest.mark.parametrize("cplx", [False, True])
def test_in_place_columns_poison_and_repeatability(hip, cplx):
    """X is Y (in place), xcol / ycol != 0, ncols = 3; NaN-poisoned neighbours stay untouched and the padding stays zero; 20 calls
    give the same bits."""
    n = 3001
    T = tc.random_triangular(n, 0.004, 29, lower=False)
    if cplx:
        T = tc.make_complex(T, 8)
    t = _tri(hip, T, False, False, 64)
    b = _rhs(n, cplx, 5, k=3)
    want = tri_solve_ref(T, b, False)
    dt = t.dtype
    # out of place, shifted columns, poisoned output block
    X = hip.alloc(n, 5, dtype=dt)
    poison(X)
    X.upload(1, b)
    Y = hip.alloc(n, 6, dtype=dt)
    poison(Y)
    hip.tri_solve(t, X, 1, Y, 2, 3)
    bits_equal(Y.download(2, 3), want, "shifted columns")
    nan = np.full((n, 1), np.nan, dtype=dt)
    if cplx:
        nan.imag = np.nan
    for c in (0, 1, 5):
        bits_equal(Y.download(c, 1), nan, "untouched column %d" % c)
    assert Y.padding_nonzero() == 0 and X.padding_nonzero() == 0
    bits_equal(X.download(1, 3), np.asfortranarray(b.astype(dt)), "the right-hand sides are not written")
    # in place
    hip.tri_solve(t, X, 1, X, 1, 3)
    bits_equal(X.download(1, 3), want, "in place")
    bits_equal(X.download(0, 1), nan, "in place: column 0")
    bits_equal(X.download(4, 1), nan, "in place: column 4")
    assert X.padding_nonzero() == 0
    # the same block, other columns
    Z = hip.alloc(n, 2, dtype=dt)
    Z.upload(0, b[:, [0]])
    s0 = hip.get("n_tri_solve")
    for _ in range(20):
        hip.tri_solve(t, Z, 0, Z, 1, 1)
        bits_equal(Z.download(1, 1), want[:, [0]], "repeat")
    assert hip.get("n_tri_solve") - s0 == 20


def _raw_csr(n, indptr, indices, data):
    M = sp.csr_matrix((n, n))
    M.indptr, M.indices, M.data = np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32), np.asarray(data, dtype=float)
    return M


@needs_single
def test_argument_errors(hip):
    from krypy_amd import _hip

    default = _default_narrow(hip)

    def refused(word, *args, **kw):
        with pytest.raises(_hip.BackendError) as e:
            hip.tri(*args, **kw)
        assert "status -2" in str(e.value) and word in str(e.value), str(e.value)

    T = tc.random_triangular(40, 0.2, 1)
    refused("wrong side", T, False)
    refused("wrong side", T.T.tocsr(), True)
    refused("no diagonal", tc.random_triangular(40, 0.2, 1, diag=False), True)
    Z = T.copy()
    Z.data[Z.indptr[6] - 1] = 0.0                  # (the diagonal is the last entry of a lower row)
    refused("zero diagonal", Z, True)
    hip.tri(Z, True, True)                         # a unit diagonal ignores it
    refused("unsorted", _raw_csr(3, [0, 1, 3, 6], [0, 1, 0, 1, 0, 2], [1, 1, 1, 1, 1, 1]), True)
    refused("duplicate", _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 0, 0, 2], [1, 1, 1, 1, 1, 1]), True)
    refused("out of range", _raw_csr(3, [0, 1, 3, 5], [0, 0, 1, 0, 7], [1, 1, 1, 1, 1]), True)
    with pytest.raises(_hip.BackendError):
        hip.tri(sp.csr_matrix(np.ones((3, 4))), True)
    # blocks that do not fit the handle
    t = hip.tri(T, True)
    tz = hip.tri(T, True, dtype=complex)
    Xr, Xz, Xs = hip.alloc(40, 1), hip.alloc(40, 1, dtype=complex), hip.alloc(39, 1)
    with pytest.raises(_hip.BackendError):
        hip.tri_solve(t, Xz, 0, Xz, 0, 1)          # real handle, complex blocks
    with pytest.raises(_hip.BackendError):
        hip.tri_solve(tz, Xr, 0, Xr, 0, 1)         # complex handle, real blocks
    with pytest.raises(_hip.BackendError):
        hip.tri_solve(t, Xr, 0, Xz, 0, 1)          # mixed
    for handle, block in ((t, Xs), (t, Xz), (tz, Xr)):      # ... and at the C boundary, which sees lengths only
        rc = hip._lib.kh_tri_solve(hip._h, handle.handle, block.handle, 0, block.handle, 0, 1)
        assert rc == -2 and b"doubles per column" in hip._lib.kh_last_error()
    with pytest.raises(_hip.BackendError) as e:
        hip.tri_solve(t, Xr, 0, Xr, 1, 1)
    assert "status -2" in str(e.value)
    with pytest.raises(_hip.BackendError):
        hip.set("tri_narrow_rows", -1)
    assert hip.get("tri_narrow_rows") == default
    # shifted column ranges of ONE block that overlap would overwrite a right-hand side before it is read: refused
    X3 = hip.alloc(40, 4)
    for xcol, ycol in ((0, 1), (1, 0), (2, 1)):
        with pytest.raises(_hip.BackendError) as e:
            hip.tri_solve(t, X3, xcol, X3, ycol, 2)
        assert "status -2" in str(e.value) and "overlap" in str(e.value)
    hip.tri_solve(t, X3, 0, X3, 2, 2)          # disjoint ranges and the identical range are fine
    hip.tri_solve(t, X3, 1, X3, 1, 3)


def test_refused_on_a_context_with_a_communicator():
    """Sharded triangular solves do not exist: a context in multi-rank mode refuses creation and says why."""
    from krypy_amd import _hip

    os.environ["KRYPY_AMD_FORCE_MULTI"] = "1"
    try:
        ctx = _hip.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
    finally:
        del os.environ["KRYPY_AMD_FORCE_MULTI"]
    try:
        with pytest.raises(_hip.BackendError) as e:
            ctx.tri(tc.bidiagonal(10), True)
        assert "status -5" in str(e.value) and "communicator" in str(e.value)
    finally:
        ctx.close()


# ---- solvers ---------------------------------------------------------------------------------------------------------
class _Twin(object):
    """Factory of the host-callable twins: ``LinearOperator(dot=oracle solve)`` - the round trip the device operators replace."""

    def __init__(self):
        self.calls = 0

    def __call__(self, T, lower=None, unit_diagonal=False):
        from krypy_amd import utils

        T = sp.csr_matrix(T)

        def dot(X):
            self.calls += X.shape[1]
            return tri_solve_ref(T, X, lower, unit_diagonal)

        return utils.LinearOperator(T.shape, T.dtype, dot=dot)


def _ilu_like(ilu, make):
    """``Pc * Uinv * Linv * Pr`` as utils.ilu_operator builds it, with `make` for the two triangular factors."""
    from krypy_amd import utils

    n = ilu.L.shape[0]
    ar = np.arange(n)
    op = make(ilu.U, lower=False) * make(ilu.L, lower=True, unit_diagonal=True)
    if not np.array_equal(ilu.perm_r, ar):
        op = op * utils.MatrixLinearOperator(sp.csr_matrix((np.ones(n), (ilu.perm_r, ar)), shape=(n, n)))
    if not np.array_equal(ilu.perm_c, ar):
        op = utils.MatrixLinearOperator(sp.csr_matrix((np.ones(n), (ar, ilu.perm_c)), shape=(n, n))) * op
    return op


def _run(solver, A, b, maxiter, **prec):
    from krypy_amd import linsys, utils

    ls = linsys.LinearSystem(A, b, **prec)
    try:
        sol = solver(ls, tol=1e-9, maxiter=maxiter)
    except utils.ConvergenceError as e:
        sol = e.solver
    return np.array(sol.resnorms), np.array(sol.xk)


def _both(hip, solver, A, b, maxiter, build, key, **flags):
    """The solver with the device operators and with their host-callable twins: the same bits; every application counted.

    Limitation: on the 300 x 200 grids the comparison covers 3 iterations (and, for the ILU cases, a coarser factorisation) only,
    because every application of the twin is a sequential Python substitution over 60,000 rows.  It shows that the wide launches
    feed a solver the oracle's bits at that size, not the behaviour of a long solve; the kernels themselves are held to the oracle
    at 70,001 rows by test_bits_of_the_sequential_substitution, and the long solves run on the 37 x 23 grids."""
    from krypy_amd import utils

    s0 = hip.get("n_tri_solve")
    res_d, x_d = _run(solver, A, b, maxiter, **dict(flags, **{key: build(utils.TriangularSolveOperator)}))
    applied = hip.get("n_tri_solve") - s0
    twin = _Twin()
    res_t, x_t = _run(solver, A, b, maxiter, **dict(flags, **{key: build(twin)}))
    bits_equal(res_d, res_t, "resnorms")
    bits_equal(x_d, x_t, "xk")
    assert applied == twin.calls and applied >= 2 * (len(res_d) - 1)
    assert hip.get("n_tri_solve") - s0 == applied          # the twin's run never touched the kernels
    return res_d


# (the large grid runs a few iterations only: every application of the twin is a sequential Python substitution over 60,000 rows)
GRIDS = [(37, 23, "natural", 60), (37, 23, "redblack", 60), (300, 200, "natural", 3), (300, 200, "redblack", 3)]


def _spilu(A):
    big = A.shape[0] > 10000
    return spla.spilu(A.tocsc(), drop_tol=5e-2 if big else 1e-3, fill_factor=1.5 if big else 4)


@needs_single
@pytest.mark.parametrize("nx,ny,order,maxiter", GRIDS)
def test_gmres_with_ilu(hip, nx, ny, order, maxiter):
    from krypy_amd import linsys, utils

    A = (tc.lap2d(nx, ny, order) + sp.diags(np.full(nx * ny - 1, 0.3), 1)).tocsr()
    ilu = _spilu(A)
    b = _rhs(nx * ny, False, 3)
    res = _both(hip, linsys.Gmres, A, b, maxiter, lambda make: _ilu_like(ilu, make), "Ml")
    assert res[-1] < res[0]
    # the public constructor builds the same operator
    got = utils.ilu_operator(ilu).dot(b)
    assert np.linalg.norm(got - ilu.solve(b[:, 0]).reshape(-1, 1)) < 1e-12 * np.linalg.norm(got)


@needs_single
@pytest.mark.parametrize("solver", ["Cg", "Minres"])
@pytest.mark.parametrize("nx,ny,order,maxiter", GRIDS)
def test_cg_minres_with_symmetric_gauss_seidel(hip, nx, ny, order, maxiter, solver):
    """M = (D + U)^{-1} D (D + L)^{-1}: symmetric positive definite, two triangular solves and a diagonal per application."""
    from krypy_amd import linsys, utils

    A = tc.lap2d(nx, ny, order)
    DL, DU = tc.triangle(A, True), tc.triangle(A, False)
    D = utils.MatrixLinearOperator(sp.diags(A.diagonal()).tocsr())
    b = _rhs(nx * ny, False, 4)
    res = _both(hip, getattr(linsys, solver), A, b, maxiter, lambda make: make(DU, lower=False) * D * make(DL, lower=True), "M",
                self_adjoint=True, positive_definite=True)
    assert res[-1] < res[0]


@needs_single
@pytest.mark.parametrize("nx,ny,order,maxiter", GRIDS)
def test_complex_gmres_with_complex_ilu(hip, nx, ny, order, maxiter):
    from krypy_amd import linsys

    n = nx * ny
    A = (tc.lap2d(nx, ny, order) - (0.4 + 0.3j) * sp.identity(n)).tocsr()
    ilu = _spilu(A)
    assert ilu.L.dtype == np.complex128
    res = _both(hip, linsys.Gmres, A, _rhs(n, True, 6), maxiter, lambda make: _ilu_like(ilu, make), "Ml")
    assert res[-1] < res[0]


@needs_single
def test_gmres_with_ilu_against_recorded_reference(hip, golden):
    """The unmodified reference's GMRES with ``Ml = LinearOperator(ilu.solve)`` on a 24 x 17 grid (tools/gen_tri_golden.py):
    the device run on the stored factors at the project's 1e-10 bar (the last entry is an explicitly formed residual)."""
    from krypy_amd import linsys, utils

    g = golden("tri_precond")
    n = int(g["n"])

    class Factors(object):
        L, U = (sp.csr_matrix((g[t + "_data"], g[t + "_indices"], g[t + "_indptr"]), shape=(n, n)) for t in "LU")
        perm_r, perm_c = g["perm_r"], g["perm_c"]

    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(n, n))
    s0 = hip.get("n_tri_solve")
    sol = linsys.Gmres(linsys.LinearSystem(A, g["b"], Ml=utils.ilu_operator(Factors)), tol=1e-8, maxiter=100)
    got, want = np.array(sol.resnorms), g["resnorms"]
    assert got.shape == want.shape
    assert np.max(np.abs(got[:-1] - want[:-1]) / want[:-1]) < 1e-10
    assert np.linalg.norm(sol.xk - g["xk"]) < 1e-10 * np.linalg.norm(g["xk"])
    assert hip.get("n_tri_solve") - s0 >= 2 * (len(want) - 1)
