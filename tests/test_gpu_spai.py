"""GPU tests of the sparse approximate inverse on a fixed pattern (krypy_amd/csrc/spai.hip): the values must be the oracle's
sequential loop (tests/support/spai_ref.py) bit for bit, and a solver preconditioned with ``utils.spai_operator`` must produce the
bits of the same solver given ``MatrixLinearOperator`` of the oracle's matrix."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import spai_cases as sc
from tests.support import tri_cases as tc
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal
from tests.support.spai_numpy_context import launch_figures
from tests.support.spai_ref import spai_ref

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
needs_single = pytest.mark.skipif(FORCED, reason="KRYPY_AMD_TEST_FORCE_MULTI=1: the context has a communicator, kh_spai_build "
                                                 "refuses (test_refused_on_a_context_with_a_communicator holds that)")

BIT_CASES = (["random_%d" % n for n in (1, 2, 63, 64, 65, 257)] + ["zrandom_%d" % n for n in (1, 2, 63, 64, 65, 257)]
             + ["lap_A", "conv_A", "zconv_A", "lap_A2", "conv_A2", "zconv_A2", "shifted_A2", "random_20001", "zrandom_20001",
                "long_row", "zlong_row", "gaps", "zgaps"])


def _check_info(info, A, P, cplx, bad=-1):
    n, qmax = A.shape[0], int(np.diff(P.indptr).max())
    W, wgs, lds = launch_figures(n, qmax, cplx)
    assert (info["n"], info["pnnz"], info["qmax"], info["first_broken_row"]) == (n, P.nnz, qmax, bad), info
    expect_kernel((info["group_width"], info["workgroups"], info["lds_bytes"]) == (W, wgs, lds), "launch figures %r, expected %r" % (info, (W, wgs, lds)))
    assert 0 < info["lds_bytes"] <= 65536


@needs_single
@pytest.mark.parametrize("name", BIT_CASES)
def test_bits_of_the_oracle(hip, name):
    """Sizes around one workgroup's rows (32 rows of 8 lanes), the 37 x 23 grid with the patterns of A (q = 5, 8 lanes per row)
    and A^2 (q = 13, 16 lanes), 20001 rows with about 7 entries each (626 workgroups), one row of exactly 32 pattern entries
    among rows of 2 and 3 (32 lanes per row for real data, 64 for complex; loops to 32 with most rows predicated off early),
    empty pattern rows and a pattern without the diagonal (r = 0 wherever row J_a does not reach column i)."""
    A, P, want, bad = sc.oracle(name)
    assert bad == -1
    cplx = A.dtype.kind == "c"
    b0 = hip.get("n_spai_build")
    m, info = hip.spai(A, P)
    bits_equal(m, want.data, name)
    _check_info(info, A, P, cplx)
    assert hip.get("n_spai_build") - b0 == 1 and hip.get("spai_device_us") > 0
    q = np.diff(P.indptr)
    if name.endswith("long_row"):
        assert info["group_width"] == (64 if cplx else 32) and q.max() == 32 and np.sort(q)[-2] == 3
    if name.endswith("gaps"):
        assert (q == 0).sum() == 3 and not np.any(P.indices == np.repeat(np.arange(A.shape[0]), q))
    if name.endswith("_A2") and "conv" in name:
        assert q.max() == 13
    if name.endswith("20001"):
        assert q.max() == 7 and (info["group_width"], info["workgroups"]) == (8, 626)


@needs_single
@pytest.mark.parametrize("name", ["conv_A2", "zconv_A2"])
def test_twenty_repeats_give_identical_bits(hip, name):
    A, P, want, _ = sc.oracle(name)
    b0 = hip.get("n_spai_build")
    for _ in range(20):
        bits_equal(hip.spai(A, P)[0], want.data, "repeat")
    assert hip.get("n_spai_build") - b0 == 20


@needs_single
@pytest.mark.parametrize("name,row", [("identical_rows", 3), ("zero_row", 8), ("zzero_row", 8), ("two_broken_rows", 3)])
def test_breakdown_is_reported_not_raised(hip, name, row):
    """The C call returns 0, names the smallest broken row and hands back what IEEE arithmetic made of it - the oracle's bits,
    the non-finite ones included; utils.spai turns it into an ArgumentError."""
    from krypy_amd import utils

    A, P, want, bad = sc.oracle(name)
    assert bad == row
    m, info = hip.spai(A, P)
    print("%s: device %s\n%s: oracle %s" % (name, [hex(v) for v in m.view(np.uint64)[~np.isfinite(m.view(np.float64))]],
                                            name, [hex(v) for v in want.data.view(np.uint64)[~np.isfinite(want.data.view(np.float64))]]))
    assert info["first_broken_row"] == row
    assert not np.all(np.isfinite(want.data))
    bits_equal(m, want.data, name)
    with pytest.raises(utils.ArgumentError) as e:
        utils.spai(A, pattern=P)
    assert "SPAI breaks down: rows of A selected by pattern row %d are linearly dependent" % row in str(e.value)


def _raw_csr(n, indptr, indices, data=None):
    M = sp.csr_matrix((n, n))
    M.indptr, M.indices = np.asarray(indptr, dtype=np.int32), np.asarray(indices, dtype=np.int32)
    M.data = np.ones(len(indices)) if data is None else np.asarray(data, dtype=float)
    return M


@needs_single
def test_argument_errors(hip):
    from krypy_amd import _hip, utils

    b0 = hip.get("n_spai_build")
    good = _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 0, 1, 2])

    def refused(word, A, P):
        with pytest.raises(_hip.BackendError) as e:
            hip.spai(A, P)
        assert "status -2" in str(e.value) and word in str(e.value), str(e.value)

    unsorted = _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 2, 0, 1])
    refused("unsorted column indices in row 2 of A", unsorted, good)
    refused("unsorted column indices in row 2 of the pattern", good, unsorted)
    refused("duplicate column indices in row 2 of the pattern", good, _raw_csr(3, [0, 1, 3, 6], [0, 0, 1, 0, 0, 2]))
    refused("column 7 out of range in row 2 of A", _raw_csr(3, [0, 1, 3, 5], [0, 0, 1, 0, 7]), good)
    refused("column 7 out of range in row 2 of the pattern", good, _raw_csr(3, [0, 1, 3, 5], [0, 0, 1, 0, 7]))
    A = sc.band(40, 17, 3)
    P = sp.csr_matrix(sp.identity(40)).tolil()
    P[21, 2:35] = 1.0
    refused("pattern row 21 has 33 entries, at most 32", A, sp.csr_matrix(P))
    with pytest.raises(_hip.BackendError):
        hip.spai(sp.csr_matrix(np.ones((3, 4))), sp.csr_matrix(np.ones((3, 4))))
    with pytest.raises(_hip.BackendError):
        hip.spai(good, sp.csr_matrix(np.ones((4, 4))))
    with pytest.raises(utils.ArgumentError) as e:
        utils.spai(A, pattern=P)
    assert "row 21" in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.spai(A, side="both")
    assert hip.get("n_spai_build") == b0          # error returns, nothing ran


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
        A = sc.convection_x(4, 3)
        with pytest.raises(_hip.BackendError) as e:
            ctx.spai(A, A)
        assert "status -5" in str(e.value) and "communicator" in str(e.value)
    finally:
        ctx.close()


# ---- solvers ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _system(nx, ny, kind):
    """(A, b, the oracle's left and right approximate inverses) - computed once, shared."""
    A = {"conv": lambda: sc.convection_x(nx, ny), "lap": lambda: tc.lap2d(nx, ny), "zconv": lambda: sc.make_complex(sc.convection_x(nx, ny), 17)}[kind]()
    rng = np.random.default_rng(3)
    b = rng.standard_normal((nx * ny, 1))
    if kind == "zconv":
        b = b + 1j * rng.standard_normal((nx * ny, 1))
    Ml, bad = spai_ref(A)
    assert bad == -1
    Mr, bad = spai_ref(A.T.tocsr())
    assert bad == -1
    Mr = Mr.T.tocsr()
    Mr.sort_indices()
    return A, b, Ml, Mr


def _run(solver, A, b, maxiter, tol, **kw):
    from krypy_amd import linsys, utils

    ls = linsys.LinearSystem(A, b, **kw)
    try:
        sol = solver(ls, tol=tol, maxiter=maxiter)
        return np.array(sol.resnorms), np.array(sol.xk), True
    except utils.ConvergenceError as e:
        return np.array(e.solver.resnorms), np.array(e.solver.xk), False


def _same_bits_and_fewer_iterations(hip, solver, A, b, key, op, twin, maxiter, tol, **flags):
    """The solver with `op` (built on the device) and with `twin` (MatrixLinearOperator of the oracle's matrix): the same bits.
    The preconditioned solve converges within `maxiter`; the plain solve given as many iterations as it took does not."""
    res_d, x_d, ok = _run(solver, A, b, maxiter, tol, **dict(flags, **{key: op}))
    res_t, x_t, _ = _run(solver, A, b, maxiter, tol, **dict(flags, **{key: twin}))
    bits_equal(res_d, res_t, "resnorms")
    bits_equal(x_d, x_t, "xk")
    assert ok, "the preconditioned solve did not converge in %d iterations" % maxiter
    its = len(res_d) - 1
    res_0, _, ok_0 = _run(solver, A, b, its, tol, **flags)
    assert not ok_0, "the plain solve needs no more than the preconditioned one's %d iterations" % its
    return its


@needs_single
@pytest.mark.parametrize("key", ["Ml", "Mr"])
@pytest.mark.parametrize("nx,ny,kind,maxiter,tol", [(37, 23, "conv", 120, 1e-8), (300, 200, "conv", 500, 1e-6), (37, 23, "zconv", 120, 1e-8)])
def test_gmres_with_spai(hip, nx, ny, kind, maxiter, tol, key):
    from krypy_amd import linsys, utils

    A, b, Ml, Mr = _system(nx, ny, kind)
    b0 = hip.get("n_spai_build")
    op = utils.spai_operator(A, side="left" if key == "Ml" else "right")
    assert hip.get("n_spai_build") - b0 == 1
    want = Ml if key == "Ml" else Mr
    bits_equal(op._A.data, want.data, "the operator's matrix")
    its = _same_bits_and_fewer_iterations(hip, linsys.Gmres, A, b, key, op, utils.MatrixLinearOperator(want), maxiter, tol)
    print("GMRES %s %dx%d %s: %d iterations" % (kind, nx, ny, key, its))


class _StepSpy(object):
    """Records the preconditioner argument of every fused Arnoldi step a context is asked for, one by one or as a whole GMRES
    cycle (kh_gmres_cycle runs the fused steps of a cycle in one C call and counts them in "n_cycle_steps")."""
    NAMES = ("arnoldi_step", "arnoldi_step_begin", "gmres_cycle")

    def __init__(self, ctx):
        self.ctx, self.kinds = ctx, []

    def __enter__(self):
        for name in self.NAMES:
            real = getattr(self.ctx, name)

            def spy(A, Md, *a, _real=real, **kw):
                self.kinds.append(None if Md is None else Md.kind)
                return _real(A, Md, *a, **kw)

            setattr(self.ctx, name, spy)
        return self

    def __exit__(self, *exc):
        for name in self.NAMES:
            delattr(self.ctx, name)


@needs_single
def test_gmres_with_spai_as_the_inner_product_preconditioner_runs_the_fused_step(hip):
    """M = spai_operator(A, symmetric=True) on the Laplacian: the Arnoldi steps are the fused step with the matrix form of Md (a
    CSR matrix) - every call that asks for steps hands the matrix over, and "n_cycle_steps", which only the fused steps inside
    kh_gmres_cycle raise, grows by the iterations; the external-operator path, a host loop that applies M through kh_apply,
    would leave both empty.  Bits of the oracle's matrix, fewer iterations than the plain solve."""
    from krypy_amd import linsys, utils

    A, b, Ml, _ = _system(37, 23, "lap")
    S = ((Ml + Ml.conj().T) / 2).tocsr()
    S.sort_indices()
    assert abs(np.linalg.eigvalsh(S.toarray()).min() - 0.083) < 5e-4
    op = utils.spai_operator(A, symmetric=True)
    bits_equal(op._A.data, S.data, "the symmetrised matrix")
    flags = dict(self_adjoint=True, positive_definite=True)
    c0 = hip.get("n_cycle_steps")
    with _StepSpy(hip) as spy:
        res, _, ok = _run(linsys.Gmres, A, b, 120, 1e-8, M=op, **flags)
    steps = hip.get("n_cycle_steps") - c0
    assert ok
    expect_kernel(len(spy.kinds) >= 1 and set(spy.kinds) == {"csr"}, "calls for fused steps with a matrix Md: kinds %r" % (spy.kinds[:8],))
    expect_kernel(steps >= len(res) - 2, "n_cycle_steps grew by %d in %d iterations" % (steps, len(res) - 1))
    its = _same_bits_and_fewer_iterations(hip, linsys.Gmres, A, b, "M", op, utils.MatrixLinearOperator(S), 120, 1e-8, **flags)
    assert its == len(res) - 1


@needs_single
@pytest.mark.parametrize("solver", ["Cg", "Minres"])
@pytest.mark.parametrize("nx,ny", [(37, 23), (300, 200)])
def test_cg_minres_with_symmetrised_spai(hip, nx, ny, solver):
    from krypy_amd import linsys, utils

    A, b, Ml, _ = _system(nx, ny, "lap")
    S = ((Ml + Ml.conj().T) / 2).tocsr()
    S.sort_indices()
    op = utils.spai_operator(A, symmetric=True)
    flags = dict(self_adjoint=True, positive_definite=True)
    tol = 1e-8 if nx == 37 else 1e-6
    its = _same_bits_and_fewer_iterations(hip, getattr(linsys, solver), A, b, "M", op, utils.MatrixLinearOperator(S), 600, tol, **flags)
    print("%s %dx%d: %d iterations" % (solver, nx, ny, its))
