"""GPU tests of the persistent ILU(0) preconditioner (krypy_amd/csrc/ilu0p.hip): the factored values and the permuted solve must be
the oracle's (tests/support/ilu0p_ref.py: ``ilu0_ref`` on ``A[p][:, p]``, then the sequential substitutions with gather and
scatter) bit for bit - for every launch plan, after every refactorisation -, and a solver preconditioned with
``utils.Ilu0Preconditioner`` must produce the bits of the same solver with a host-callable twin built from the oracle."""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import ilu0_cases as ic
from tests.support import tri_cases as tc
from tests.support.ilu0p_ref import Ilu0pRef, permuted
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal, poison, poisoned_allocations
from tests.support.tri_ref import levels_ref

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
needs_single = pytest.mark.skipif(FORCED, reason="KRYPY_AMD_TEST_FORCE_MULTI=1: the context has a communicator, kh_ilu0_create "
                                                 "refuses (test_refused_on_a_context_with_a_communicator holds that)")
_default = {}
_i32p = ctypes.POINTER(ctypes.c_int32)
_f64p = ctypes.POINTER(ctypes.c_double)


def _default_narrow(ctx):
    """The library's own default of tri_narrow_rows, read once before this module sets anything."""
    if id(ctx) not in _default:
        _default[id(ctx)] = ctx.get("tri_narrow_rows")
    return _default[id(ctx)]


def _handle(ctx, A, perm=None, narrow=None):
    default = _default_narrow(ctx)
    ctx.set("tri_narrow_rows", default if narrow is None else narrow)
    try:
        return ctx.ilu0_handle(A, perm, dtype=A.dtype)
    finally:
        ctx.set("tri_narrow_rows", default)


def _solve(ctx, h, b):
    """Out of place into a poisoned block."""
    X = ctx.upload(b, dtype=h.dtype)
    Y = poison(ctx.alloc(b.shape[0], b.shape[1], dtype=h.dtype, zero=False))
    ctx.ilu0_solve(h, X, 0, Y, 0, b.shape[1])
    return Y.download()


def _rhs(n, cplx, seed, k=1):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, k))
    return b + 1j * rng.standard_normal((n, k)) if cplx else b


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


def _multicolor(A):
    from krypy_amd import _hip

    G = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    G = (G + G.T).tocsr()
    G.sort_indices()
    color, nc = _hip.multicolor(G)
    return np.argsort(color, kind="stable"), nc


def band_plus_one(n, seed):
    """Tridiagonal plus one random off-band entry per row, strictly diagonally dominant (so ILU(0) exists under every symmetric
    permutation): diagonal >= 3.25 against at most 1.125 + 1.0625 + 0.5."""
    if n == 1:
        return sp.csr_matrix(np.array([[3.5]]))
    rng = np.random.default_rng(seed)
    rows, cols = np.arange(n), rng.integers(0, n, size=n)
    keep = np.abs(rows - cols) > 1
    R = sp.csr_matrix((rng.uniform(-0.5, 0.5, keep.sum()), (rows[keep], cols[keep])), shape=(n, n))
    A = (ic.tridiagonal(n) + sp.identity(n) + R).tocsr()
    A.sort_indices()
    return A


CASES = {
    "random20001": lambda: ic.random_dominant(20001, 77, per_row=6),
    "convection": lambda: ic.convection(37, 23),
    "nine_point": lambda: ic.nine_point(37, 23),
}
for _n in (1, 2, 63, 64, 65, 129, 4097):
    CASES["band%d" % _n] = functools.partial(band_plus_one, _n, 40 + _n)


@functools.lru_cache(maxsize=None)
def _case(name, ordering, cplx):
    """(A, perm or None, the oracle, rows per level of L, of U): computed once, shared, never written."""
    A = CASES[name]()
    if cplx:
        A = ic.make_complex(A, 3)
    n = A.shape[0]
    perm = {"natural": lambda: None, "random": lambda: np.random.default_rng(n).permutation(n), "multicolor": lambda: _multicolor(A)[0]}[ordering]()
    ref = Ilu0pRef(A, perm)
    assert ref.bad == -1
    cnt_l = levels_ref(sp.tril(ref.Ap, -1).tocsr(), True)[1]
    cnt_u = levels_ref(sp.triu(ref.Ap, 0).tocsr(), False)[1]
    return A, perm, ref, cnt_l, cnt_u


def _check_bits(hip, name, ordering, cplx, narrow=None, k=2):
    A, perm, ref, cnt_l, cnt_u = _case(name, ordering, cplx)
    n = A.shape[0]
    h = _handle(hip, A, perm, narrow)
    c0 = [hip.get(key) for key in ("n_ilu0p_refactor", "n_ilu0p_solve", "n_ilu0p_wide", "n_ilu0p_narrow")]
    info = hip.ilu0_refactor(h, A.data)
    what = "%s %s cplx=%s narrow=%s" % (name, ordering, cplx, narrow)
    assert info["first_broken_row"] == -1 and (info["n"], info["nnz"], info["levels"]) == (n, A.nnz, len(cnt_l))
    assert info["widest_level"] == cnt_l.max() and info["longest_row"] == int(np.diff(A.indptr).max())
    bits_equal(h.values(), ref.values, what + " values")
    b = _rhs(n, cplx, 11, k)
    bits_equal(_solve(hip, h, b), ref.solve(b), what + " solve")
    # info() and the launch counters against the host plan
    nr = _default_narrow(hip) if narrow is None else narrow
    (fw, fn), (uw, un) = _plan(cnt_l, nr), _plan(cnt_u, nr)
    hi = h.info()
    assert (hi["n"], hi["nnz"], hi["levels"], hi["levels_l"], hi["levels_u"]) == (n, A.nnz, len(cnt_l), len(cnt_l), len(cnt_u))
    assert hi["permuted"] == (perm is not None) and hi["factored"] and hi["device_bytes"] >= 8 * A.nnz * (2 if cplx else 1)
    expect_kernel((hi["wide_launches"], hi["narrow_launches"], hi["solve_wide_launches"], hi["solve_narrow_launches"]) == (fw, fn, fw + uw, fn + un),
                  "%s: plan %r, expected %r" % (what, hi, (fw, fn, fw + uw, fn + un)))
    c1 = [hip.get(key) for key in ("n_ilu0p_refactor", "n_ilu0p_solve", "n_ilu0p_wide", "n_ilu0p_narrow")]
    expect_kernel([a - b for a, b in zip(c1, c0)] == [1, k, fw + k * (fw + uw), fn + k * (fn + un)], "%s: counters" % what)
    return h


# ---- device bits against the oracle ---------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "random"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 4097])
def test_bits_of_the_oracle_around_the_slice_boundaries(hip, n, ordering, cplx):
    """Tridiagonal plus one random off-band entry per row, with and without a random permutation: sizes around the slice (64)
    boundary, and 4097 rows."""
    _check_bits(hip, "band%d" % n, ordering, cplx)


@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_bits_of_the_oracle_on_a_random_pattern(hip, ordering, cplx):
    """A random nonsymmetric pattern with a diagonal, about 7 entries per row, 20001 rows: several workgroups per level; the
    multicolour ordering of its own colouring."""
    A, perm, ref, cnt_l, cnt_u = _case("random20001", ordering, cplx)
    assert 6.0 < A.nnz / 20001.0 < 8.0 and cnt_l.max() > 256
    _check_bits(hip, "random20001", ordering, cplx, k=1)


@needs_single
@pytest.mark.parametrize("narrow", [0, 64, 1024])
@pytest.mark.parametrize("name,ordering,levels", [("convection", "natural", 59), ("convection", "multicolor", 2), ("nine_point", "multicolor", 4)])
def test_grids_under_every_launch_plan(hip, name, ordering, levels, narrow):
    """The 37 x 23 five-point convection-diffusion grid under both orderings (59 levels, 2 levels) and the nine-point grid under
    the multicolour ordering (4 colours), each under tri_narrow_rows 0, 64 and 1024, real and complex."""
    for cplx in (False, True):
        _, _, _, cnt_l, cnt_u = _case(name, ordering, cplx)
        assert len(cnt_l) == levels == len(cnt_u)
        _check_bits(hip, name, ordering, cplx, narrow)
    if ordering == "multicolor":
        assert _multicolor(CASES[name]())[1] == levels


# ---- refactorisation ----------------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_refactorisation_on_one_handle(hip, ordering, cplx):
    """One handle, three value sets on the 37 x 23 pattern: after each, values and solve are a fresh handle's and the oracle's;
    one creation; one upload of nnz values and 4 bytes back per refactorisation."""
    A0 = ic.convection(37, 23)
    perm = _multicolor(A0)[0] if ordering == "multicolor" else None
    w = 2 if cplx else 1
    b = _rhs(A0.shape[0], cplx, 2)
    c0 = hip.get("n_ilu0p_create")
    h = _handle(hip, ic.make_complex(A0, 1) if cplx else A0, perm, 64)
    assert hip.get("n_ilu0p_create") - c0 == 1 and not h.info()["factored"]
    for wind in (0.8, 1.2, 1.6):
        A = ic.convection(37, 23, wind=wind)
        if cplx:
            A = ic.make_complex(A, 1)
        assert np.array_equal(A.indices, A0.indices)
        info = hip.ilu0_refactor(h, A.data)
        assert info["first_broken_row"] == -1
        assert (hip.get("ilu0p_h2d_bytes"), hip.get("ilu0p_d2h_bytes")) == (A.nnz * 8 * w, 4)
        assert hip.get("n_ilu0p_create") - c0 == 1
        ref = Ilu0pRef(A, perm)
        got_v, got_x = h.values(), _solve(hip, h, b)
        bits_equal(got_v, ref.values, "values, wind %g" % wind)
        bits_equal(got_x, ref.solve(b), "solve, wind %g" % wind)
        fresh = _handle(hip, A, perm, 64)
        hip.ilu0_refactor(fresh, A.data)
        bits_equal(got_v, fresh.values(), "values against a fresh handle")
        bits_equal(got_x, _solve(hip, fresh, b), "solve against a fresh handle")
        del fresh
        c0 += 1          # (the fresh handle's creation)
    r0 = hip.get("n_ilu0p_refactor")
    for _ in range(20):
        hip.ilu0_refactor(h, A.data)
        bits_equal(h.values(), got_v, "repeat: values")
        bits_equal(_solve(hip, h, b), got_x, "repeat: solve")
    assert hip.get("n_ilu0p_refactor") - r0 == 20 and hip.get("ilu0p_refactor_us") >= 0


# ---- breakdown --------------------------------------------------------------------------------------------------------------
@needs_single
def test_breakdown_leaves_the_handle_unfactored_until_a_good_refactorisation(hip):
    """A zero PIVOT (IEEE arithmetic: 1 / 0 = inf, nothing faults): the 3 x 3 case and two zero pivots in different levels."""
    B = sp.csr_matrix(np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, 3]]))
    Bgood = sp.csr_matrix(np.array([[1.0, 1, 0], [1, 3, 1], [0, 1, 3]]))
    A = ic.two_zero_pivots()
    Agood = ic.with_values(A, {(15, 15): 3.0, (30, 30): 2.0})
    rev = np.arange(39, -1, -1)
    for bad_m, good_m, perm, narrow, row in ((B, Bgood, None, 0, 1), (B, Bgood, None, None, 1), (A, Agood, None, 0, 15), (A, Agood, None, 64, 15),
                                             (A, Agood, rev, 0, Ilu0pRef(A, rev).bad)):
        n = bad_m.shape[0]
        assert row >= 0
        h = _handle(hip, bad_m, perm, narrow)
        X = hip.upload(_rhs(n, False, 1))
        lu = np.empty(bad_m.nnz)
        for attempt in range(2):          # never refactored, then broken down
            rc = hip._lib.kh_ilu0_solve(hip._h, h.handle, X.handle, 0, X.handle, 0, 1)
            assert rc == -2 and b"not factored" in hip._lib.kh_last_error()
            rc = hip._lib.kh_ilu0_values(h.handle, lu.ctypes.data_as(_f64p))
            assert rc == -2 and b"not factored" in hip._lib.kh_last_error()
            assert not h.info()["factored"]
            if attempt == 0:
                assert hip.ilu0_refactor(h, bad_m.data)["first_broken_row"] == row
        assert hip.ilu0_refactor(h, good_m.data)["first_broken_row"] == -1 and h.info()["factored"]
        fresh = _handle(hip, good_m, perm, narrow)
        hip.ilu0_refactor(fresh, good_m.data)
        ref = Ilu0pRef(good_m, perm)
        b = _rhs(n, False, 3)
        bits_equal(h.values(), fresh.values(), "revived: values")
        bits_equal(h.values(), ref.values, "revived: the oracle's values")
        bits_equal(_solve(hip, h, b), _solve(hip, fresh, b), "revived: solve")
        bits_equal(_solve(hip, h, b), ref.solve(b), "revived: the oracle's solve")


# ---- in place and shifted columns -----------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_in_place_shifted_columns_and_padding(hip, ordering, cplx):
    """X is Y (in place), different columns of one block ((W, 0, W, 1) as the solvers call M), ncols = 3, blocks with ld > n (851
    rows); NaN-poisoned neighbours stay untouched and rows [n, ld) stay zero; overlapping ranges are refused; the same on blocks
    from a poisoned pool."""
    from krypy_amd import _hip

    A, perm, ref, _, _ = _case("convection", ordering, cplx)
    n = A.shape[0]
    h = _handle(hip, A, perm, 64)
    hip.ilu0_refactor(h, A.data)
    b = _rhs(n, cplx, 5, k=3)
    want = ref.solve(b)
    dt = h.dtype
    nan = np.full((n, 1), np.nan, dtype=dt)
    if cplx:
        nan.imag = np.nan
    with poisoned_allocations(hip):
        X = poison(hip.alloc(n, 5, dtype=dt, zero=False))
        X.upload(1, b)
        Y = poison(hip.alloc(n, 6, dtype=dt, zero=False))
        hip.ilu0_solve(h, X, 1, Y, 2, 3)
        bits_equal(Y.download(2, 3), want, "shifted columns")
        for c in (0, 1, 5):
            bits_equal(Y.download(c, 1), nan, "untouched column %d" % c)
        assert Y.padding_nonzero() == 0 and X.padding_nonzero() == 0
        bits_equal(X.download(1, 3), np.asfortranarray(b.astype(dt)), "the right-hand sides are not written")
        hip.ilu0_solve(h, X, 1, X, 1, 3)          # in place
        bits_equal(X.download(1, 3), want, "in place")
        bits_equal(X.download(0, 1), nan, "in place: column 0")
        bits_equal(X.download(4, 1), nan, "in place: column 4")
        assert X.padding_nonzero() == 0
        W = poison(hip.alloc(n, 2, dtype=dt, zero=False))          # (W, 0, W, 1)
        W.upload(0, b[:, [0]])
        hip.ilu0_solve(h, W, 0, W, 1, 1)
        bits_equal(W.download(1, 1), want[:, [0]], "the same block, the next column")
        bits_equal(W.download(0, 1), np.asfortranarray(b[:, [0]].astype(dt)), "the same block: the right-hand side")
        assert W.padding_nonzero() == 0
    X3 = hip.alloc(n, 4, dtype=dt)
    for xcol, ycol in ((0, 1), (1, 0), (2, 1)):
        with pytest.raises(_hip.BackendError) as e:
            hip.ilu0_solve(h, X3, xcol, X3, ycol, 2)
        assert "status -2" in str(e.value) and "overlap" in str(e.value)
    hip.ilu0_solve(h, X3, 0, X3, 2, 2)          # disjoint ranges and the identical range are fine
    hip.ilu0_solve(h, X3, 1, X3, 1, 3)


# ---- argument errors through the C ABI ----------------------------------------------------------------------------------------------
def _create(hip, n, indptr, indices, perm=None, cplx=0):
    indptr = None if indptr is None else np.asarray(indptr, dtype=np.int32)
    indices = None if indices is None else np.asarray(indices, dtype=np.int32)
    perm = None if perm is None else np.asarray(perm, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(_i32p)
    h = ctypes.c_void_p()
    rc = hip._lib.kh_ilu0_create(hip._h, n, 0 if indices is None else indices.size, ptr(indptr), ptr(indices), ptr(perm), cplx, ctypes.byref(h))
    return rc, hip._lib.kh_last_error().decode(), h


@needs_single
def test_argument_errors(hip):
    from krypy_amd import _hip

    c0 = hip.get("n_ilu0p_create")
    good = ([0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2])
    for word, args in (("NULL array", (3, None, good[1])), ("NULL array", (3, good[0], None)),
                       ("perm is not a permutation of 0 .. n-1 (entry 2)", (3,) + good + ([0, 1, 1],)),
                       ("perm is not a permutation of 0 .. n-1 (entry 0)", (3,) + good + ([3, 1, 0],)),
                       ("perm is not a permutation of 0 .. n-1 (entry 1)", (3,) + good + ([2, -1, 0],)),
                       ("unsorted column indices in row 2", (3, [0, 1, 3, 6], [0, 0, 1, 2, 0, 1])),
                       ("duplicate column indices in row 2", (3, [0, 1, 3, 6], [0, 0, 1, 0, 0, 2])),
                       ("column 7 out of range in row 2", (3, [0, 1, 3, 5], [0, 0, 1, 0, 7])),
                       ("row 1 has no diagonal entry", (3, [0, 2, 3, 5], [0, 1, 0, 1, 2]))):
        rc, msg, _ = _create(hip, *args)
        assert rc == -2 and word in msg and msg.startswith("kh_ilu0_create"), (word, rc, msg)
    assert hip._lib.kh_ilu0_create(hip._h, 3, 7, None, None, None, 0, None) == -2
    assert hip.get("n_ilu0p_create") == c0          # error returns, nothing was created
    with pytest.raises(_hip.BackendError):
        hip.ilu0_handle(sp.csr_matrix(np.ones((3, 4))))
    # NULL values, NULL info; solve before refactor
    A = ic.convection(7, 5)
    h, hz = hip.ilu0_handle(A), hip.ilu0_handle(A, dtype=complex)
    info = (ctypes.c_int64 * 8)()
    assert hip._lib.kh_ilu0_refactor(hip._h, h.handle, None, info) == -2 and b"NULL" in hip._lib.kh_last_error()
    assert hip._lib.kh_ilu0_refactor(hip._h, h.handle, A.data.ctypes.data_as(_f64p), None) == -2
    assert hip._lib.kh_ilu0_info(h.handle, None) == -2 and hip._lib.kh_ilu0_values(h.handle, None) == -2
    Xr, Xz, Xs = hip.alloc(35, 1), hip.alloc(35, 1, dtype=complex), hip.alloc(34, 1)
    with pytest.raises(_hip.BackendError) as e:
        hip.ilu0_solve(h, Xr, 0, Xr, 0, 1)
    assert "status -2" in str(e.value) and "not factored" in str(e.value)
    hip.ilu0_refactor(h, A.data)
    hip.ilu0_refactor(hz, A.data)
    with pytest.raises(_hip.BackendError):
        hip.ilu0_solve(h, Xz, 0, Xz, 0, 1)          # real handle, complex blocks
    with pytest.raises(_hip.BackendError):
        hip.ilu0_solve(hz, Xr, 0, Xr, 0, 1)         # complex handle, real blocks
    with pytest.raises(_hip.BackendError):
        hip.ilu0_refactor(h, A.data * 1j)
    with pytest.raises(_hip.BackendError):
        hip.ilu0_refactor(h, A.data[:-1])
    for handle, block in ((h, Xs), (h, Xz), (hz, Xr)):      # ... and at the C boundary, which sees lengths only
        rc = hip._lib.kh_ilu0_solve(hip._h, handle.handle, block.handle, 0, block.handle, 0, 1)
        assert rc == -2 and b"doubles per column" in hip._lib.kh_last_error()
    assert hip._lib.kh_ilu0_solve(hip._h, h.handle, None, 0, Xr.handle, 0, 1) == -2
    assert hip._lib.kh_ilu0_solve(hip._h, h.handle, Xr.handle, 0, Xr.handle, 1, 1) == -2          # column 1 of a block with 1
    # a foreign context
    other = _hip.Context(0)
    try:
        rc = hip._lib.kh_ilu0_solve(other._h, h.handle, Xr.handle, 0, Xr.handle, 0, 1)
        assert rc == -2 and b"another context" in hip._lib.kh_last_error()
        rc = hip._lib.kh_ilu0_refactor(other._h, h.handle, A.data.ctypes.data_as(_f64p), info)
        assert rc == -2 and b"another context" in hip._lib.kh_last_error()
    finally:
        other.close()
    hip.ilu0_solve(h, Xr, 0, Xr, 0, 1)          # the handle is as good as before


def test_refused_on_a_context_with_a_communicator():
    """Sharded factorisations do not exist: a context in multi-rank mode refuses and says why."""
    from krypy_amd import _hip

    os.environ["KRYPY_AMD_FORCE_MULTI"] = "1"
    try:
        ctx = _hip.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
    finally:
        del os.environ["KRYPY_AMD_FORCE_MULTI"]
    try:
        with pytest.raises(_hip.BackendError) as e:
            ctx.ilu0_handle(ic.tridiagonal(10))
        assert "status -5" in str(e.value) and "communicator" in str(e.value)
    finally:
        ctx.close()


# ---- solvers ---------------------------------------------------------------------------------------------------------
def _run(solver, A, b, maxiter, tol=1e-9, **kw):
    from krypy_amd import linsys, utils

    ls = linsys.LinearSystem(A, b, **kw)
    try:
        sol = solver(ls, tol=tol, maxiter=maxiter)
        return np.array(sol.resnorms), np.array(sol.xk), True
    except utils.ConvergenceError as e:
        return np.array(e.solver.resnorms), np.array(e.solver.xk), False


@functools.lru_cache(maxsize=None)
def _grid_oracle(kind, nx, ny, ordering, cplx):
    A = tc.lap2d(nx, ny) if kind == "lap2d" else ic.convection(nx, ny)
    if cplx:
        A = ic.make_complex(A, 9)
    perm = ic.redblack_permutation(nx, ny) if ordering == "multicolor" else None
    ref = Ilu0pRef(A, perm)
    assert ref.bad == -1
    return A, ref


def _against_twin(hip, solver, kind, nx, ny, ordering, cplx, maxiter, key, **flags):
    """The solver with utils.Ilu0Preconditioner and with the host-callable twin of the oracle: the same bits, every application
    counted.  On the 300 x 200 grid the comparison covers 2 iterations only - every application of the twin is a sequential
    Python substitution over 60,000 rows -; the long solves run on the 37 x 23 grid."""
    from krypy_amd import utils

    A, ref = _grid_oracle(kind, nx, ny, ordering, cplx)
    b = _rhs(nx * ny, cplx, 3)
    s0, c0 = hip.get("n_ilu0p_solve"), hip.get("n_ilu0p_create")
    M = utils.Ilu0Preconditioner(A, ordering)
    if ordering == "multicolor":
        assert np.array_equal(M._perm, ref.perm) and M.info["colors"] == 2
    res_d, x_d, _ = _run(solver, A, b, maxiter, **dict(flags, **{key: M}))
    applied = hip.get("n_ilu0p_solve") - s0
    assert hip.get("n_ilu0p_create") - c0 == 1
    calls = [0]

    def dot(X):
        calls[0] += X.shape[1]
        return ref.solve(X)

    twin = utils.LinearOperator(A.shape, A.dtype, dot=dot)
    res_t, x_t, _ = _run(solver, A, b, maxiter, **dict(flags, **{key: twin}))
    bits_equal(res_d, res_t, "resnorms")
    bits_equal(x_d, x_t, "xk")
    assert applied == calls[0] and applied >= len(res_d) - 1
    assert res_d[-1] < res_d[0]
    return A, b, M


def _iterations(solver, A, b, key, op, maxiter, **flags):
    res, _, ok = _run(solver, A, b, maxiter, tol=1e-8, **dict(flags, **({key: op} if op is not None else {})))
    return len(res) - 1, ok


def _same_count_as_the_composed_operator_and_fewer_than_plain(solver, A, b, key, M, ordering, maxiter, **flags):
    from krypy_amd import utils

    its, ok = _iterations(solver, A, b, key, M, maxiter, **flags)
    assert ok, "the preconditioned solve did not converge in %d iterations" % maxiter
    assert _iterations(solver, A, b, key, utils.ilu0_operator(A, ordering), maxiter, **flags) == (its, True)
    _, ok0 = _iterations(solver, A, b, key, None, its, **flags)
    assert not ok0, "the plain solve needs no more than the preconditioned one's %d iterations" % its


@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
@pytest.mark.parametrize("key", ["Ml", "Mr"])
@pytest.mark.parametrize("nx,ny,maxiter", [(37, 23, 120), (300, 200, 2)])
def test_gmres_with_the_preconditioner(hip, nx, ny, maxiter, key, ordering, cplx):
    from krypy_amd import linsys

    A, b, M = _against_twin(hip, linsys.Gmres, "convection", nx, ny, ordering, cplx, maxiter, key)
    _same_count_as_the_composed_operator_and_fewer_than_plain(linsys.Gmres, A, b, key, M, ordering, 120 if nx == 37 else 600)


@needs_single
@pytest.mark.parametrize("solver", ["Cg", "Minres"])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
@pytest.mark.parametrize("nx,ny,maxiter", [(37, 23, 80), (300, 200, 2)])
def test_cg_minres_with_the_preconditioner(hip, nx, ny, maxiter, ordering, solver):
    """On a symmetric A ILU(0) is L D L^T: M is symmetric positive definite up to rounding."""
    from krypy_amd import linsys

    flags = dict(self_adjoint=True, positive_definite=True)
    A, b, M = _against_twin(hip, getattr(linsys, solver), "lap2d", nx, ny, ordering, False, maxiter, "M", **flags)
    _same_count_as_the_composed_operator_and_fewer_than_plain(getattr(linsys, solver), A, b, "M", M, ordering, 80 if nx == 37 else 600,
                                                              **flags)


# ---- a sequence ------------------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_a_sequence_of_systems_on_one_pattern(hip, ordering):
    """Three systems, the convection coefficient scaled by 1, 1.5, 2, solved with ONE preconditioner and update() between them:
    each solve is the solve with a freshly constructed preconditioner, bit for bit; one creation, three refactorisations."""
    from krypy_amd import linsys, utils

    b = _rhs(37 * 23, False, 7)
    c0, r0 = hip.get("n_ilu0p_create"), hip.get("n_ilu0p_refactor")
    M = None
    got = []
    for scale in (1.0, 1.5, 2.0):
        A = ic.convection(37, 23, wind=0.8 * scale)
        if M is None:
            M = utils.Ilu0Preconditioner(A, ordering)
        else:
            M.update(A)
        got.append(_run(linsys.Gmres, A, b, 120, Ml=M))
    assert (hip.get("n_ilu0p_create") - c0, hip.get("n_ilu0p_refactor") - r0) == (1, 3)
    assert M.info["refactorisations"] == 3
    for scale, (res, x, ok) in zip((1.0, 1.5, 2.0), got):
        A = ic.convection(37, 23, wind=0.8 * scale)
        res_f, x_f, ok_f = _run(linsys.Gmres, A, b, 120, Ml=utils.Ilu0Preconditioner(A, ordering))
        assert ok and ok_f
        bits_equal(res, res_f, "resnorms, scale %g" % scale)
        bits_equal(x, x_f, "xk, scale %g" % scale)
