"""CPU tests of the block-Jacobi preconditioner: the oracle (tests/support/bjac_ref.py) against independent facts, and the Python
layer (``utils.block_jacobi``, ``utils.BlockJacobiPreconditioner``, ``utils.block_jacobi_operator``) on a NumPy context whose
``bjac_create`` / ``bjac_update`` / ``bjac_apply`` / ``bjac_values`` are the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bjac_cases as bc
from tests.support.bjac_ref import apply_ref, bjac_ref, coupled, gauss_jordan
from tests.support.poison import bits_equal

EPS = np.finfo(np.float64).eps

# max |B^-1 B - I| / (eps cond_inf(B)) of the oracle over the blocks of test_oracle_against_numpy_inv (measured: 0.50, at a
# complex block; 0.46 over the real ones).  The test holds ten times that: NumPy's own rounding of the product and of the
# condition number differs between builds.
ORACLE_RESIDUAL = 0.50


@pytest.fixture
def bjac_double():
    from krypy_amd import _hip
    from tests.support.bjac_numpy_context import BjacNumpyContext

    ctx = BjacNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


# ---- the oracle against independent facts ------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_against_numpy_inv(cplx):
    """The generator's blocks, every m in 1 .. 32, five of each."""
    rng = np.random.RandomState(7)
    worst = 0.0
    for m in range(1, 33):
        for _ in range(5):
            B = bc.random_block(rng, m, cplx)
            inv, broken = gauss_jordan(B)
            assert not broken and inv.dtype == B.dtype
            cond = np.linalg.cond(B, np.inf)
            worst = max(worst, float(np.abs(inv @ B - np.eye(m)).max()) / (EPS * float(np.abs(cond))))
            err = np.abs(inv - np.linalg.inv(B)).max() / np.abs(inv).max()
            assert err <= 10 * 3.1 * EPS * np.linalg.cond(B), (m, err)
    print("max |inv B - I| / (eps cond_inf) = %.3f (%s)" % (worst, "complex" if cplx else "real"))
    assert worst <= 10 * ORACLE_RESIDUAL, worst


@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_row_swap_ties_and_broken_blocks(cplx):
    one = (1.0 + 0j) if cplx else 1.0
    inv, broken = gauss_jordan(np.array([[0.0, 1.0], [1.0, 0.0]]) * one)
    assert not broken and np.array_equal(inv, np.array([[0.0, 1.0], [1.0, 0.0]]))
    # equal magnitudes in a column: the smallest row at or below the diagonal is the pivot
    for B, want in ((np.array([[2.0, 1.0], [-2.0, 1.0]]), [0, 1]),
                    (np.array([[1.0, 0, 0], [-1.0, 1, 0], [1.0, 0, 1]]), [0, 1, 2]),
                    (np.array([[0.5, 1.0, 0], [1.0, 0, 3], [-1.0, 0, 1]]), [1, 1, 2]),       # rows 1 and 2 tie in column 0
                    (np.array([[0.0, 1.0, 0], [0.0, 0, 3], [-1.0, 0, 1]]), [2, 2, 2])):
        piv = []
        inv, broken = gauss_jordan(B * one, pivots=piv)
        assert not broken and piv == want, (B, piv)
        assert np.abs(inv @ B - np.eye(B.shape[0])).max() <= 8 * EPS
    if cplx:          # the magnitude is |re| + |im|: 0.5 + 0.5j ties with 1 and with -1j
        piv = []
        gauss_jordan(np.array([[0.5 + 0.5j, 1.0], [-1j, 2.0]]), pivots=piv)
        assert piv == [0, 1]
    for B in (np.array([[1.0, 2.0], [2.0, 4.0]]), np.zeros((2, 2)), np.zeros((1, 1)), np.array([[1.0, np.nan], [0.0, 1.0]]),
              np.array([[np.inf]])):
        assert gauss_jordan(B.astype(complex) if cplx else B)[1], B
    assert not gauss_jordan(np.array([[1e-300, 1.0], [1.0, 1.0]]) * one)[1]


@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_pivot_cases_invert(cplx):
    """Anti-diagonal blocks, tied columns and the 1e-300 diagonals are regular: the oracle's inverse is an inverse."""
    for name, (A, ptr) in bc.pivot_cases(cplx).items():
        values, blocks, bad = bjac_ref(A, ptr)
        assert bad == -1, name
        for g, inv in enumerate(blocks):
            B = A[ptr[g]:ptr[g + 1], ptr[g]:ptr[g + 1]].toarray()
            assert np.abs(inv @ B - np.eye(B.shape[0])).max() <= 64 * EPS * np.linalg.cond(B, np.inf), (name, g)


@pytest.mark.parametrize("cplx", [False, True])
def test_oracle_apply_is_the_csr_product_order(cplx):
    """The apply sum is scipy's csr_matvec order on the assembled block-diagonal matrix for real data (separate multiply and
    add, rising columns); for complex data it is that order with the product taken part by part."""
    from krypy_amd import precond as utils          # (_bjac_csr is private to the module the preconditioners live in)

    ptr = bc.cycle_ptr(40)
    A = bc.block_system(ptr, 3, cplx)
    values, blocks, bad = bjac_ref(A, ptr)
    M = utils._bjac_csr(values, ptr, A.shape[0])
    x = bc.rhs(A.shape[0], 1, cplx, 4)[:, 0]
    y = apply_ref(blocks, ptr, x)
    if not cplx:
        bits_equal(y, M.dot(x), "apply")
    assert np.abs(y - M.dot(x)).max() <= 64 * EPS * np.abs(M).dot(np.abs(x)).max()


# ---- the Python layer on the double ------------------------------------------------------------------------------------
def test_block_size_one_is_the_reciprocal_diagonal(bjac_double):
    from krypy_amd import utils

    A = coupled(5, 4, 3, seed=1)
    M = utils.block_jacobi(A, block_size=1)
    bits_equal(M.diagonal(), 1.0 / A.diagonal(), "1 / diag")
    assert M.nnz == A.shape[0] and M.info["group_width"] == 1 and M.info["nblk"] == A.shape[0]


@pytest.mark.parametrize("cplx", [False, True])
def test_block_jacobi_assembles_the_csr_matrix(bjac_double, cplx):
    from krypy_amd import utils

    ptr = bc.cycle_ptr(37)
    A = bc.block_system(ptr, 9, cplx)
    n = A.shape[0]
    M = utils.block_jacobi(A, blocks=ptr)
    values, blocks, bad = bjac_ref(A, ptr)
    assert sp.isspmatrix_csr(M) and M.shape == A.shape and M.has_sorted_indices and M.dtype == A.dtype
    m = np.diff(ptr)
    assert M.nnz == int((m.astype(np.int64) ** 2).sum())
    want = sp.block_diag(blocks, format="csr")
    pattern = sp.block_diag([np.ones((k, k)) for k in m], format="csr")
    assert np.array_equal(M.indptr, pattern.indptr) and np.array_equal(M.indices, pattern.indices)
    bits_equal(M.toarray(), want.toarray().astype(A.dtype), "blocks")
    bits_equal(M.data, values, "data order")
    assert M.info["first_broken_block"] == -1 and M.info["max_block"] == 32 and M.info["group_width"] == 32 and M.info["n"] == n
    # block_size: the last block is shorter
    M4 = utils.block_jacobi(A, block_size=4)
    assert M4.info["nblk"] == -(-n // 4) and M4.nnz == (n // 4) * 16 + (n % 4) ** 2


def test_operator_forms_agree_and_update(bjac_double):
    from krypy_amd import utils

    A = coupled(6, 5, 4, seed=2)
    n = A.shape[0]
    Pb = utils.block_jacobi_operator(A, block_size=4)
    Pm = utils.block_jacobi_operator(A, block_size=4, form="matrix")
    assert isinstance(Pb, utils.BlockJacobiPreconditioner) and isinstance(Pm, utils.MatrixLinearOperator)
    assert Pb._device_matrix() is None and Pb.info["builds"] == 1 and Pb.info["nblk"] == n // 4
    bits_equal(Pb.matrix().toarray(), Pm._A.toarray(), "matrix()")
    x = bc.rhs(n, 3, False, 1)
    assert np.abs(Pb.dot(x) - Pm._A.dot(x)).max() <= 64 * EPS * np.abs(Pm._A).dot(np.abs(x)).max()
    with pytest.raises(utils.LinearOperatorError):          # no adjoint
        Pb.dot_adj(x)
    # update: the same pattern, new values
    A2 = A.copy()
    A2.data = A2.data * np.random.RandomState(3).uniform(0.5, 1.5, A2.nnz)
    Pb.update(A2)
    assert Pb.info["builds"] == 2 and bjac_double.calls["bjac_update"] == 1
    bits_equal(Pb.matrix().toarray(), utils.block_jacobi(A2, block_size=4).toarray(), "updated")
    # another pattern, shape or kind of values is refused
    A3 = sp.csr_matrix(A + sp.csr_matrix(([1.0], ([0], [n - 1])), shape=A.shape))
    for bad in (A3, coupled(6, 5, 2, seed=2), A.astype(np.complex128)):
        with pytest.raises(utils.ArgumentError):
            Pb.update(bad)
    # a broken update leaves the object unusable until one succeeds
    A4 = A.copy()
    A4.data[:] = 0.0
    with pytest.raises(utils.ArgumentError) as e:
        Pb.update(A4)
    assert "block 0" in str(e.value)
    with pytest.raises(utils.LinearOperatorError):
        Pb.dot(x)
    Pb.update(A)
    bits_equal(Pb.matrix().toarray(), Pm._A.toarray(), "recovered")


def test_argument_checks(bjac_double):
    from krypy_amd import utils

    A = coupled(4, 3, 2, seed=1)
    n = A.shape[0]
    for kw in (dict(), dict(block_size=2, blocks=[0, n]), dict(block_size=0), dict(block_size=33), dict(block_size=2.0),
               dict(block_size=True), dict(blocks=[1, n]), dict(blocks=[0, n - 1]), dict(blocks=[0, 4, 4, n]),
               dict(blocks=[0, 8, 4, n]), dict(blocks=[0.0, float(n)]), dict(blocks=[0]), dict(blocks=[[0, n]])):
        for fn in (utils.block_jacobi, utils.BlockJacobiPreconditioner, utils.block_jacobi_operator):
            with pytest.raises(utils.ArgumentError):
                fn(A, **kw)
    big = sp.identity(40, format="csr")
    with pytest.raises(utils.ArgumentError) as e:
        utils.block_jacobi(big, blocks=[0, 3, 36, 40])
    assert "block 1" in str(e.value) and "33" in str(e.value)
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi(sp.csr_matrix(np.ones((3, 4))), block_size=1)
    with pytest.raises(utils.ArgumentError):
        utils.block_jacobi_operator(A, block_size=2, form="dense")
    # a broken block is named, the smallest one
    B = A.tolil()
    B[6, :] = 0
    B[2, :] = 0
    B = sp.csr_matrix(B)
    B.eliminate_zeros()
    for fn in (utils.block_jacobi, utils.BlockJacobiPreconditioner):
        with pytest.raises(utils.ArgumentError) as e:
            fn(B, block_size=2)
        assert "block 1 " in str(e.value) and "rows 2 .. 3" in str(e.value)
    assert bjac_double.calls.get("bjac_apply", 0) == 0


def test_as_preconditioner_of_the_solvers(bjac_double):
    """Ml of GMRES on the double: block-Jacobi needs far fewer iterations than point Jacobi on the coupled system."""
    from krypy_amd import linsys, utils

    A = coupled(6, 5, 4, seed=2)
    n = A.shape[0]
    b = np.ones((n, 1))
    its = {}
    for name, Ml in (("block", utils.block_jacobi_operator(A, block_size=4)),
                     ("matrix", utils.block_jacobi_operator(A, block_size=4, form="matrix")),
                     ("point", utils.block_jacobi_operator(A, block_size=1, form="matrix"))):
        try:
            sol = linsys.Gmres(linsys.LinearSystem(A, b, Ml=Ml), tol=1e-8, maxiter=n)
        except utils.ConvergenceError as e:
            sol = e.solver
        its[name] = len(sol.resnorms) - 1
        if name != "point":
            assert np.linalg.norm(b - A.dot(sol.xk)) / np.linalg.norm(b) <= 1e-7
    assert its["block"] == its["matrix"] and 2 * its["block"] <= its["point"], its
