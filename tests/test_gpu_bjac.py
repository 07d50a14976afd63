"""GPU tests of the block-Jacobi preconditioner (krypy_amd/csrc/bjac.hip): the inverses must be the oracle's Gauss-Jordan
elimination (tests/support/bjac_ref.py) bit for bit at every group width, the apply kernel must give the oracle's sum and the bits
of the library's CSR SpMV on the assembled block-diagonal matrix, and solvers preconditioned with either form must agree."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bjac_cases as bc
from tests.support.bjac_ref import apply_ref, bjac_ref, coupled, group_width
from tests.support.poison import bits_equal, poison

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
needs_single = pytest.mark.skipif(FORCED, reason="KRYPY_AMD_TEST_FORCE_MULTI=1: the context has a communicator, kh_bjac_create "
                                                 "refuses (test_refused_on_a_context_with_a_communicator holds that)")


def _nan_aware_bits(got, want, what):
    """Bit for bit where the oracle has a number; a NaN where it has a NaN (sign and payload of a NaN are the processor's)."""
    got, want = np.asarray(got), np.asarray(want)
    g, w = got.reshape(-1).view(np.float64), want.reshape(-1).view(np.float64)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), "%s: NaN at other places" % what
    bits_equal(np.where(nan, 0.0, g), np.where(nan, 0.0, w), what)


def _check_build(hip, A, ptr, what, broken=-1):
    """One create: values, info and counters against the oracle.  Returns (handle, oracle blocks)."""
    want, blocks, bad = bjac_ref(A, ptr)
    assert bad == broken, (what, bad)
    b0 = hip.get("n_bjac_build")
    h, info = hip.bjac_create(A, ptr)
    got = hip.bjac_values(h)
    if broken < 0:
        bits_equal(got, want, what)
    else:
        _nan_aware_bits(got, want, what)
    m = np.diff(ptr)
    W = group_width(int(m.max()))
    tiles = -(-m.size // (64 // W))
    assert (info["n"], info["nnz"], info["nblk"], info["max_block"], info["group_width"], info["first_broken_block"]) == \
        (A.shape[0], A.nnz, m.size, int(m.max()), W, broken), (what, info)
    assert info["workgroups"] == min(-(-tiles // 4), hip.info()["reduce_blocks"]) and info["device_bytes"] > 0
    assert hip.get("n_bjac_build") - b0 == 1 and h.info() == info
    return h, blocks


def _apply(hip, h, x, ncols_block=None, xcol=0, ycol=0):
    """Applies the handle to the columns of the host array x through poisoned blocks; returns (Y host, Y block)."""
    n, k = x.shape
    X = hip.alloc(n, (ncols_block or k) + xcol, dtype=h.dtype)
    X.upload(xcol, np.asfortranarray(x))
    Y = poison(hip.alloc(n, (ncols_block or k) + ycol + 1, dtype=h.dtype, zero=False))
    hip.bjac_apply(h, X, xcol, Y, ycol, k)
    return Y.download(), Y


# ---- 1. / 2. build bits ---------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("bs", bc.UNIFORM_SIZES)
def test_build_bits_uniform_blocks(hip, bs, cplx):
    """Every group width at its full size and one above the width below; 1, 64/W - 1, 64/W, 64/W + 1 and 256/W + 1 blocks (one
    tile short of, exactly and past a wave, past a workgroup); n one short of a multiple, so the last block is shorter.  The
    apply on the same handle must be the oracle's sum."""
    for nblk in bc.uniform_counts(bs):
        A, ptr = bc.uniform_case(bs, nblk, cplx)
        what = "bs=%d nblk=%d" % (bs, nblk)
        h, blocks = _check_build(hip, A, ptr, what)
        x = bc.rhs(A.shape[0], 1, cplx, nblk)
        y, _ = _apply(hip, h, x)
        bits_equal(y[:, 0], apply_ref(blocks, ptr, x[:, 0]), what + " apply")


@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("part", ["cycle", "lone32"])
def test_build_bits_variable_blocks(hip, part, cplx):
    """Sizes cycling through 1 .. 32 (W = 32, two blocks per wave, most lanes idle in most groups), and one block of 32
    between blocks of 1."""
    ptr = bc.cycle_ptr(70) if part == "cycle" else bc.lone_32_ptr()
    A = bc.block_system(ptr, 21, cplx)
    h, blocks = _check_build(hip, A, ptr, part)
    x = bc.rhs(A.shape[0], 1, cplx, 2)
    y, _ = _apply(hip, h, x)
    bits_equal(y[:, 0], apply_ref(blocks, ptr, x[:, 0]), part + " apply")


# ---- 3. pivoting ----------------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", ["antidiagonal", "ties", "tiny"])
def test_pivoting(hip, name, cplx):
    """A swap at every step; equal magnitudes in a column (the smallest row wins, or the bits differ); 1e-300 on the diagonal
    beside entries of order 1."""
    A, ptr = bc.pivot_cases(cplx)[name]
    _check_build(hip, A, ptr, name)


# ---- 4. extraction --------------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
def test_extraction_and_broken_blocks(hip, cplx):
    """In-block entries missing, many entries left and right of the block, a row without an entry inside its block, an empty
    row, a NaN: three broken blocks, the smallest is reported, every other block has the oracle's bits (a NaN is a NaN where
    the oracle has one).  The Python layer names the block."""
    from krypy_amd import utils

    A, ptr, broken = bc.extraction_case(cplx)
    assert np.diff(A.indptr).max() >= 85 and np.diff(A.indptr).min() == 0
    _check_build(hip, A, ptr, "extraction", broken=broken[0])
    for fn in (utils.block_jacobi, utils.BlockJacobiPreconditioner):
        with pytest.raises(utils.ArgumentError) as e:
            fn(A, blocks=ptr)
        assert "block 2 " in str(e.value) and "rows 10 .. 14" in str(e.value)
    # with the broken blocks repaired one at a time the next one is reported
    B = A.tolil()
    B[13, 13] = 7.0
    _check_build(hip, bc.canonical(B.tocsr()), ptr, "extraction, block 2 repaired", broken=broken[1])
    B[21, 21] = 7.0
    _check_build(hip, bc.canonical(B.tocsr()), ptr, "extraction, blocks 2 and 4 repaired", broken=broken[2])
    B[32, 31] = 0.5
    _check_build(hip, bc.canonical(B.tocsr()), ptr, "extraction, all repaired")


# ---- 5. apply bits --------------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("bs", [3, 4, 8, 17, 32])
def test_apply_bits_of_the_oracle_and_of_the_csr_spmv(hip, bs, cplx):
    """The apply kernel against the oracle's sum and against ``ctx.apply`` of the CSR matrix from ``block_jacobi`` (the library's
    SpMV, with and without its banded copy) bit for bit; one column and three columns at column offsets; the poisoned
    neighbouring columns keep their NaNs and the padding rows [n, ld) of Y (n is odd: ld > n) stay what they were - zero, the
    library's invariant for every block, so a write there would show only if it were not a zero; the kernel's row guard is
    ``i < m_g``."""
    from krypy_amd import utils

    nblk = 3 * 256 // group_width(bs) + 2
    n = nblk * bs - 1 if (nblk * bs) % 2 == 0 else nblk * bs
    ptr = bc.uniform_ptr(n, bs)
    A = bc.block_system(ptr, 77 + bs, cplx)
    M = utils.block_jacobi(A, blocks=ptr)
    want, blocks, _ = bjac_ref(A, ptr)
    bits_equal(M.data, want, "block_jacobi")
    P = utils.BlockJacobiPreconditioner(A, blocks=ptr)
    h = P._device_handle(hip)
    Md = hip.csr(M)
    a0 = hip.get("n_bjac_apply")
    for k, xcol, ycol in ((1, 0, 0), (3, 2, 1)):
        x = bc.rhs(n, k, cplx, 10 + k)
        ref = np.column_stack([apply_ref(blocks, ptr, x[:, c]) for c in range(k)])
        y, Y = _apply(hip, h, x, xcol=xcol, ycol=ycol)
        bits_equal(y[:, ycol:ycol + k], ref, "apply against the oracle")
        rest = [c for c in range(Y.ncols) if not ycol <= c < ycol + k]
        assert np.all(np.isnan(y[:, rest])), "a neighbouring column was written"
        assert Y.padding_nonzero() == 0 and (cplx or Y.ld > n)
        for dia in (1, 0):
            hip.set("spmv_dia", dia)
            try:
                X = hip.upload(np.asfortranarray(x), dtype=h.dtype)
                Z = poison(hip.alloc(n, k, dtype=h.dtype, zero=False))
                hip.apply(Md, X, 0, Z, 0, k)
                bits_equal(Z.download(), ref, "the CSR SpMV (spmv_dia=%d)" % dia)
            finally:
                hip.set("spmv_dia", 1)
        bits_equal(P.dot(x), ref, "LinearOperator.dot")
    assert hip.get("n_bjac_apply") - a0 == 2 * (1 + 3)


# ---- 6. striding ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def reduce_blocks(hip):
    nb0 = hip.info()["reduce_blocks"]
    try:
        yield lambda nb: hip.tune(reduce_blocks=nb)
    finally:
        hip.tune(reduce_blocks=nb0)


@needs_single
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("W", [4, 32])
def test_three_workgroups_stride(hip, reduce_blocks, W, cplx):
    """reduce_blocks = 3 and 2 * 3 * 256 / W + 1 blocks: every workgroup takes two rounds and one wave a third; the bits of the
    default grid."""
    ptr = bc.stride_ptr(W)
    A = bc.block_system(ptr, 5, cplx)
    x = bc.rhs(A.shape[0], 1, cplx, 6)
    h, info = hip.bjac_create(A, ptr)
    assert info["workgroups"] == 2 * 3 + 1
    v0 = hip.bjac_values(h)
    y0, _ = _apply(hip, h, x)
    reduce_blocks(3)
    assert hip.info()["reduce_blocks"] == 3
    h3, info3 = hip.bjac_create(A, ptr)
    assert info3["workgroups"] == 3
    bits_equal(hip.bjac_values(h3), v0, "values, three workgroups")
    y3, _ = _apply(hip, h3, x)
    bits_equal(y3, y0, "apply, three workgroups")
    y03, _ = _apply(hip, h, x)
    bits_equal(y03, y0, "apply of the first handle, three workgroups")
    want, blocks, _ = bjac_ref(A, ptr)
    bits_equal(v0, want, "values")
    bits_equal(y0[:, 0], apply_ref(blocks, ptr, x[:, 0]), "apply")


# ---- 7. update ------------------------------------------------------------------------------------------------------------
@needs_single
@pytest.mark.parametrize("cplx", [False, True])
def test_update_is_a_fresh_build(hip, cplx):
    from krypy_amd import utils

    ptr = bc.cycle_ptr(45)
    A = bc.block_system(ptr, 31, cplx)
    A2 = A.copy()
    A2.data = A2.data * np.random.RandomState(2).uniform(0.5, 1.5, A2.nnz)
    P = utils.BlockJacobiPreconditioner(A, blocks=ptr)
    b0 = hip.get("n_bjac_build")
    P.update(A2)
    first = P.matrix()
    P.update(A2)
    assert hip.get("n_bjac_build") - b0 == 2 and P.info["builds"] == 3 and hip.get("bjac_device_us") >= 0
    fresh = utils.block_jacobi(A2, blocks=ptr)
    bits_equal(first.data, fresh.data, "update against a fresh build")
    bits_equal(P.matrix().data, first.data, "the same update twice")
    bits_equal(fresh.data, bjac_ref(A2, ptr)[0], "the fresh build against the oracle")
    x = bc.rhs(A.shape[0], 2, cplx, 3)
    bits_equal(P.dot(x), utils.BlockJacobiPreconditioner(A2, blocks=ptr).dot(x), "apply after update")
    with pytest.raises(utils.ArgumentError):
        P.update(bc.block_system(ptr, 31, cplx, off=3))


# ---- 8. solves ------------------------------------------------------------------------------------------------------------
def _run(solver, A, b, maxiter=2000, tol=1e-8, **kw):
    from krypy_amd import linsys, utils

    skw = {k: kw.pop(k) for k in list(kw) if k == "s"}
    ls = linsys.LinearSystem(A, b, **kw)
    try:
        sol = solver(ls, tol=tol, maxiter=maxiter, **skw)
        return np.array(sol.resnorms), np.array(sol.xk), True
    except utils.ConvergenceError as e:
        return np.array(e.solver.resnorms), np.array(e.solver.xk), False


@functools.lru_cache(maxsize=None)
def _coupled(m, seed):
    A = coupled(12, 10, m, seed=seed)
    return A, np.ones((A.shape[0], 1))


SYSTEMS = [(4, 2), (8, 1)]


@needs_single
@pytest.mark.parametrize("m,seed", SYSTEMS)
@pytest.mark.parametrize("how", ["Gmres-Ml", "Gmres-Mr", "Bicgstab-Ml", "Idrs-Ml"])
def test_solves_with_both_forms(hip, how, m, seed):
    """``coupled(12, 10, 4, seed=2)`` and ``coupled(12, 10, 8, seed=1)``, b = ones, tol = 1e-8: the two forms apply the same
    arithmetic, so residual norms and iterate agree bit for bit; the true residual is at most 1e-7 (the solver's tolerance is
    on the preconditioned residual; the same runs on the NumPy double give 1.4e-9 .. 1.3e-8).  GMRES with block-Jacobi needs
    at most half the iterations of GMRES with point Jacobi (33 against 418 and 36 against 522 on the double)."""
    from krypy_amd import linsys, utils

    A, b = _coupled(m, seed)
    name, side = how.split("-")
    kw = dict(s=4) if name == "Idrs" else {}
    S = getattr(linsys, name)
    out = {}
    for form in ("blocks", "matrix"):
        op = utils.block_jacobi_operator(A, block_size=m, form=form)
        out[form] = _run(S, A, b, **dict(kw, **{side: op}))
        res, x, ok = out[form]
        r = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
        print("%s %s m=%d: %d iterations, ||b - A x|| / ||b|| = %.3e" % (how, form, m, len(res) - 1, r))
        assert ok and r <= 1e-7, (form, r)
    bits_equal(out["blocks"][0], out["matrix"][0], "resnorms")
    bits_equal(out["blocks"][1], out["matrix"][1], "xk")
    if how == "Gmres-Ml":
        point = sp.diags(1.0 / A.diagonal()).tocsr()
        res_p, _, _ = _run(S, A, b, Ml=utils.MatrixLinearOperator(point))
        print("point Jacobi: %d iterations" % (len(res_p) - 1))
        assert 2 * (len(out["blocks"][0]) - 1) <= len(res_p) - 1, (len(out["blocks"][0]) - 1, len(res_p) - 1)


@needs_single
def test_cg_on_a_hermitian_positive_definite_system(hip):
    """S = A^T A + I of a small coupled system: M = block-Jacobi in both forms, both converge to tol."""
    from krypy_amd import linsys, utils

    A = coupled(6, 5, 4, seed=2)
    S = bc.canonical(A.T @ A + sp.identity(A.shape[0]))
    b = np.ones((S.shape[0], 1))
    spd = dict(self_adjoint=True, positive_definite=True)
    its = {}
    for form in ("matrix", "blocks"):
        res, x, ok = _run(linsys.Cg, S, b, M=utils.block_jacobi_operator(S, 4, form=form), **spd)
        assert ok and res[-1] <= 1e-8, (form, res[-1])
        assert np.linalg.norm(b - S @ x) / np.linalg.norm(b) <= 1e-7
        its[form] = len(res) - 1
    res0, _, _ = _run(linsys.Cg, S, b, **spd)
    assert its["blocks"] < len(res0) - 1, (its, len(res0) - 1)


@needs_single
def test_complex_gmres(hip):
    """A + 0.5j I with complex block-Jacobi as Ml, both forms."""
    from krypy_amd import linsys, utils

    A, b = _coupled(4, 2)
    Az = bc.canonical(A + 0.5j * sp.identity(A.shape[0]))
    bz = b.astype(np.complex128)
    out = {}
    for form in ("blocks", "matrix"):
        out[form] = _run(linsys.Gmres, Az, bz, Ml=utils.block_jacobi_operator(Az, block_size=4, form=form))
        res, x, ok = out[form]
        assert ok and np.linalg.norm(bz - Az @ x) / np.linalg.norm(bz) <= 1e-7
    bits_equal(out["blocks"][0], out["matrix"][0], "resnorms")
    bits_equal(out["blocks"][1], out["matrix"][1], "xk")


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------
def test_refused_on_a_context_with_a_communicator():
    """Sharded blocks do not exist: a context in multi-rank mode refuses and says why."""
    from krypy_amd import _hip

    os.environ["KRYPY_AMD_FORCE_MULTI"] = "1"
    try:
        ctx = _hip.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
    finally:
        del os.environ["KRYPY_AMD_FORCE_MULTI"]
    try:
        A, ptr = bc.uniform_case(4, 3, False)
        with pytest.raises(_hip.BackendError) as e:
            ctx.bjac_create(A, ptr)
        assert "status -5" in str(e.value) and "communicator" in str(e.value)
    finally:
        ctx.close()


@needs_single
def test_refusals(hip):
    from krypy_amd import _hip, utils

    A, ptr = bc.uniform_case(4, 9, False)
    n = A.shape[0]
    b0 = hip.get("n_bjac_build")
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi(sp.csr_matrix(np.ones((3, 4))), block_size=2)
    with pytest.raises(_hip.BackendError):
        hip.bjac_create(sp.csr_matrix(np.ones((3, 4))), [0, 3])
    for bad, word in (([0, 33, n], "block 0"), ([0, 4, n - 1], "not at n"), ([0, 4, n + 1], "block"), ([1, 4, n], "start at 0"),
                      ([0, 8, 8, n], "block 1"), ([0, 8, 4, n], "block 1")):
        with pytest.raises(_hip.BackendError) as e:
            hip.bjac_create(sp.identity(n, format="csr"), np.array(bad))
        assert "status -2" in str(e.value) and word in str(e.value), str(e.value)
    big = sp.identity(40, format="csr")
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi(big, blocks=[0, 33, 40])
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi(big, blocks=[0, 20, 39])
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi(big, block_size=4, blocks=[0, 20, 40])
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi(big)
    # unsorted indices and a column out of range, the row named
    U = sp.csr_matrix((np.ones(4), np.array([0, 2, 1, 2], dtype=np.int32), np.array([0, 1, 3, 4], dtype=np.int32)), shape=(3, 3))
    with pytest.raises(_hip.BackendError) as e:
        hip.bjac_create(U, [0, 3])
    assert "row 1" in str(e.value)
    assert hip.get("n_bjac_build") == b0          # error returns, nothing ran
    # a real handle on complex blocks, the reverse, overlapping columns of one block, another length
    h, _ = hip.bjac_create(A, ptr)
    hz, _ = hip.bjac_create(A.astype(np.complex128), ptr)
    a0 = hip.get("n_bjac_apply")
    Xr, Xz = hip.alloc(n, 4), hip.alloc(n, 4, dtype=np.complex128)
    for hh, X in ((h, Xz), (hz, Xr)):
        with pytest.raises(_hip.BackendError) as e:
            hip.bjac_apply(hh, X, 0, X, 2, 1)
        assert "status -2" in str(e.value)
    for xcol, ycol, k in ((0, 0, 1), (0, 1, 2), (2, 1, 2)):
        with pytest.raises(_hip.BackendError) as e:
            hip.bjac_apply(h, Xr, xcol, Xr, ycol, k)
        assert "status -2" in str(e.value) and "overlap" in str(e.value)
    with pytest.raises(_hip.BackendError):
        hip.bjac_apply(h, hip.alloc(n + 1, 1), 0, hip.alloc(n + 1, 1), 0, 1)
    with pytest.raises(_hip.BackendError):
        hip.bjac_apply(h, Xr, 3, hip.alloc(n, 2), 0, 2)
    assert hip.get("n_bjac_apply") == a0
    hip.bjac_apply(h, Xr, 0, Xr, 2, 2)          # disjoint ranges of one block are fine
    assert hip.get("n_bjac_apply") - a0 == 2
