"""BiCGStab on the device: the step kernels at their edges (k_bicg_dir / _half / _dots / _full behind ``bicgstab_step`` and
the three separate entries), the clamps, and whole solves on both paths of ``linsys.Bicgstab``."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bicgstab_cases as bc
from tests.support import bicgstab_ref as ref
from tests.support import poison
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

FORCED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") == "1"
needs_single = pytest.mark.skipif(FORCED, reason="KRYPY_AMD_TEST_FORCE_MULTI=1: the context has a communicator, the ILU(0) "
                                                 "factorisation and the SPAI build refuse (their own tests hold that)")

RT, R, P, V, S, T, Y = range(7)          # the columns of a state block
BETA, OMEGA_PREV = 0.625, -0.375


def random_csr(n, seed):
    """about five entries per row anywhere in the row, plus a diagonal of 4: not symmetric; canonical CSR"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 5)
    A = sp.csr_matrix((rng.standard_normal(5 * n), (rows, rng.integers(0, n, 5 * n))), shape=(n, n))
    A = sp.csr_matrix(A + 4.0 * sp.identity(n))
    A.sum_duplicates()
    A.sort_indices()
    return A


def banded_csr(n, seed):
    """three diagonals with random entries at offsets -1, 0, 2 (cheap to build at two million rows)"""
    rng = np.random.default_rng(seed)
    return sp.csr_matrix(sp.diags([rng.standard_normal(n - 1), 4.0 + rng.standard_normal(n), rng.standard_normal(n - 2)],
                                  [-1, 0, 2]))


def random_state(n, seed):
    rng = np.random.default_rng(seed)
    H = np.zeros((n, 7), order="F")
    for c in (RT, R, P, V, Y):
        H[:, c] = rng.standard_normal(n)
    return H


def sum_bound(a, b):
    """2 n 2^-53 sum |a_i b_i|: the worst case of any summation order, doubled for the rounding of the products"""
    return 2.0 * a.size * 2.0 ** -53 * float(np.sum(np.abs(a.astype(np.longdouble) * b.astype(np.longdouble))))


def ld_dot(a, b):
    return np.sum(a.astype(np.longdouble) * b.astype(np.longdouble))


def step(hip, Amat, B, rho, first=False):
    return hip.bicgstab_step(Amat, B, RT, B, R, B, P, B, V, B, S, B, T, B, Y, first, BETA, OMEGA_PREV, rho)


def check_step(hip, A, upload, csr):
    """One ``bicgstab_step`` from a random state: the six sums against extended precision on the device's own vectors,
    the vectors against ``step_ref`` fed the device's sums (bit for bit), the operator products against SciPy (CSR), and
    the same bits from a second call on the same state."""
    n = A.shape[0]
    H0 = random_state(n, 11 + n % 1000)
    rho = 0.8125
    Amat = upload(A)
    B = hip.upload(H0)
    out = step(hip, Amat, B, rho)
    H = B.download()
    sigma, ss, theta, phi, rho_new, rr, flags = out
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(H))
    assert flags == ref.flags_of(rho, sigma, theta, phi, rho_new)      # (n = 1: r = s - (ts / tt) t may be exactly 0)
    pairs = {"sigma": (sigma, H[:, RT], H[:, V]), "ss": (ss, H[:, S], H[:, S]), "theta": (theta, H[:, T], H[:, S]),
             "phi": (phi, H[:, T], H[:, T]), "rho_new": (rho_new, H[:, RT], H[:, R]), "rr": (rr, H[:, R], H[:, R])}
    for name, (got, a, b) in pairs.items():
        err, bound = abs(float(np.longdouble(got) - ld_dot(a, b))), sum_bound(a, b)
        print("n = %d %s: error %.3e, bound %.3e" % (n, name, err, bound))
        assert err <= bound, (name, n, err, bound)
    state = dict(apply=A.dot, r=H0[:, R], p=H0[:, P], v=H0[:, V], y=H0[:, Y])
    scal = dict(first=False, beta=BETA, omega_prev=OMEGA_PREV, rho=rho, sigma=sigma, theta=theta, phi=phi)
    want = ref.step_ref(state, scal, v=None if csr else H[:, V], t=None if csr else H[:, T])
    for name, c in (("p", P), ("v", V), ("s", S), ("t", T), ("y", Y), ("r", R)):
        poison.bits_equal(H[:, c], want[name], "n = %d: %s" % (n, name))
    poison.bits_equal(H[:, RT], H0[:, RT], "rt is left as it was")
    assert not B.padding_nonzero()
    B2 = hip.upload(H0)
    out2 = step(hip, Amat, B2, rho)
    assert out2 == out
    poison.bits_equal(B2.download(), H, "second call on the same state")
    return out


@pytest.fixture
def reduce_blocks(hip):
    nb0 = hip.info()["reduce_blocks"]

    def tune(nb):
        if nb:
            hip.tune(reduce_blocks=nb)
        return hip

    try:
        yield tune
    finally:
        hip.tune(reduce_blocks=nb0)


# ---- step tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3, 0])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 4097])
def test_step_sparse(reduce_blocks, n, nb):
    ctx = reduce_blocks(nb)
    check_step(ctx, random_csr(n, n), ctx.csr, csr=True)


def test_step_dense(hip):
    check_step(hip, random_csr(257, 5).toarray(), hip.dense, csr=False)


def test_step_banded(hip):
    check_step(hip, bc.convdiff(37, 23, 1.0, 0.3), hip.csr, csr=True)


def test_step_largest_grid(reduce_blocks):
    """reduce_blocks = 4096 and n = 8192 * 256 + 1: grid_lin would launch 8192 workgroups; the two-sum kernels run on 4096
    and their second sum's last partial is the last double of the partial space (the layout in bicgstab.hip)."""
    ctx = reduce_blocks(4096)
    assert ctx.info()["reduce_blocks"] == 4096
    check_step(ctx, banded_csr(8192 * 256 + 1, 3), ctx.csr, csr=True)


def test_step_writes_before_it_reads(hip):
    """v, s, t from ``zero=False`` allocations full of NaN: nothing returned or stored is touched by them"""
    n = 1023
    A = random_csr(n, 2)
    H0 = random_state(n, 4)
    Amat = hip.csr(A)
    blocks = [hip.upload(H0[:, c]) for c in (RT, R, P)]
    with poison.poisoned_allocations(hip) as rec:
        v, s, t = (hip.alloc(n, 1, zero=False) for _ in range(3))
    assert rec.poisoned == 3
    y = hip.upload(H0[:, Y])
    rt, r, p = blocks
    out = hip.bicgstab_step(Amat, rt, 0, r, 0, p, 0, v, 0, s, 0, t, 0, y, 0, True, 0.0, 0.0, 1.25)
    assert np.all(np.isfinite(out))
    for b in (rt, r, p, v, s, t, y):
        assert np.all(np.isfinite(b.download())) and not b.padding_nonzero()
    poison.bits_equal(p.download()[:, 0], H0[:, P], "first = True leaves p as it is")
    poison.bits_equal(v.download()[:, 0], A.dot(H0[:, P]), "v = A p")


@pytest.mark.parametrize("kind", ["csr", "dense", "diag"])
def test_pieces_are_the_step(hip, kind):
    """bicgstab_dir + apply + bicgstab_half + apply + bicgstab_full leave the bits of bicgstab_step"""
    n = 1023
    A = random_csr(n, 9)
    Amat = {"csr": lambda: hip.csr(A), "dense": lambda: hip.dense(A.toarray()), "diag": lambda: hip.diag(A.diagonal())}[kind]()
    H0 = random_state(n, 6)
    rho = -0.75
    B = hip.upload(H0)
    out = step(hip, Amat, B, rho)
    C = hip.upload(H0)
    hip.bicgstab_dir(C, R, C, P, C, V, BETA, OMEGA_PREV)
    hip.apply(Amat, C, P, C, V)
    sigma, ss, f0 = hip.bicgstab_half(C, RT, C, R, C, V, C, S, rho)
    hip.apply(Amat, C, S, C, T)
    theta, phi, rho_new, rr, f1 = hip.bicgstab_full(C, RT, C, R, C, P, C, S, C, T, C, Y)
    assert (sigma, ss, theta, phi, rho_new, rr, f0 | f1) == out
    poison.bits_equal(C.download(), B.download(), "pieces against the step")
    # theta_known: <t, s> is taken from the context's scratch scalar, where the call above left it, and only phi is summed
    D = hip.upload(H0)
    hip.bicgstab_dir(D, R, D, P, D, V, BETA, OMEGA_PREV)
    hip.apply(Amat, D, P, D, V)
    assert hip.bicgstab_half(D, RT, D, R, D, V, D, S, rho) == (sigma, ss, f0)
    hip.apply(Amat, D, S, D, T)
    assert hip.bicgstab_full(D, RT, D, R, D, P, D, S, D, T, D, Y, theta_known=True) == (theta, phi, rho_new, rr, f1)
    poison.bits_equal(D.download(), B.download(), "theta_known = 1 against the step")


def test_clamps_on_the_device(hip):
    """The zero operator: v = 0, sigma = 0 clamps alpha to 0 and s = r; t = 0, 0 / 0 clamps omega and r = s; nothing
    becomes inf or nan"""
    from krypy_amd import _hip
    n = 300
    H0 = random_state(n, 8)
    B = hip.upload(H0)
    out = step(hip, hip.diag(np.zeros(n)), B, 1.5, first=True)
    H = B.download()
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(out)) and out[0] == 0.0 and out[2] == 0.0 and out[3] == 0.0
    assert out[6] == _hip.BICG_ALPHA_CLAMPED | _hip.BICG_OMEGA_CLAMPED
    poison.bits_equal(H[:, S], H0[:, R], "alpha = 0: s = r")
    poison.bits_equal(H[:, R], H0[:, R], "omega = 0: r = s")
    poison.bits_equal(H[:, Y], H0[:, Y], "no step: y as it was")


def test_argument_errors(hip):
    from krypy_amd._hip import BackendError
    n = 64
    A = hip.csr(random_csr(n, 1))
    B = hip.upload(random_state(n, 1))
    short = hip.alloc(n - 1, 1)
    with pytest.raises(BackendError, match="same column"):
        hip.bicgstab_step(A, B, RT, B, R, B, P, B, V, B, S, B, S, B, Y, False, 1.0, 1.0, 1.0)
    with pytest.raises(BackendError, match="length mismatch"):
        hip.bicgstab_step(A, B, RT, B, R, B, P, B, V, B, S, B, T, short, 0, False, 1.0, 1.0, 1.0)
    with pytest.raises(BackendError, match="length mismatch"):
        hip.bicgstab_step(hip.csr(random_csr(n - 1, 1)), B, RT, B, R, B, P, B, V, B, S, B, T, B, Y, False, 1.0, 1.0, 1.0)
    with pytest.raises(BackendError, match="real operator"):
        hip.bicgstab_step(hip.csr(random_csr(n, 1).astype(complex)), B, RT, B, R, B, P, B, V, B, S, B, T, B, Y, False, 1.0, 1.0,
                          1.0)
    with pytest.raises(BackendError, match="column of its own"):
        hip.bicgstab_dir(B, R, B, R, B, V, 1.0, 1.0)
    with pytest.raises(BackendError, match="length mismatch"):
        hip.bicgstab_dir(B, R, short, 0, B, V, 1.0, 1.0)
    with pytest.raises(BackendError, match="column of its own"):
        hip.bicgstab_half(B, RT, B, R, B, V, B, V, 1.0)
    with pytest.raises(BackendError, match="length mismatch"):
        hip.bicgstab_half(B, RT, B, R, B, V, short, 0, 1.0)
    with pytest.raises(BackendError, match="column of its own"):
        hip.bicgstab_full(B, RT, B, R, B, P, B, S, B, T, B, P)
    with pytest.raises(BackendError, match="column of its own"):
        hip.bicgstab_full(B, RT, B, S, B, P, B, S, B, T, B, Y)
    with pytest.raises(BackendError, match="length mismatch"):
        hip.bicgstab_full(B, RT, B, R, B, P, B, S, short, 0, B, Y)
    with pytest.raises(BackendError):
        hip.bicgstab_dir(B, R, B, P, hip.alloc(n, 1, dtype=np.complex128), 0, 1.0, 1.0)


# ---- clamp and breakdown, whole solves (the cases of tests/test_bicgstab_host.py on the device) ------------------------
def test_multiple_of_identity(hip):
    bc.case_multiple_of_identity()


def test_swap_breakdown(hip):
    bc.case_swap_breakdown()


@pytest.mark.parametrize("name", sorted(bc.SYSTEMS))
def test_whole_solve(hip, name):
    c0 = hip.get("n_bicgstab_steps")
    sol = bc.case_whole_solve(name)
    expect_kernel(hip.get("n_bicgstab_steps") - c0 == sol.iter, "one bicgstab_step call per iteration: %r" % name)


def test_initial_guess(hip):
    bc.case_initial_guess()


def test_shapes(hip):
    bc.case_shapes()


def test_zero_rhs(hip):
    bc.case_zero_rhs()


def test_maxiter(hip):
    bc.case_maxiter()


@pytest.mark.parametrize("side", ["Ml", "Mr"])
def test_generic_path(hip, side):
    made = bc.case_generic(side, lambda: hip.get("n_bicgstab_steps"))
    expect_kernel(made == 0, "the generic path makes no bicgstab_step call (%s)" % side)


@needs_single
def test_device_preconditioners(hip):
    """ILU(0) from the left and SPAI from the right: both converge in fewer iterations than the plain solve"""
    from krypy_amd import utils
    A, b = bc.scaled_system()
    plain = bc.solve(A, b)
    c0 = hip.get("n_bicgstab_steps")
    left = bc.solve(A, b, Ml=utils.ilu0_operator(A))
    right = bc.solve(A, b, Mr=utils.spai_operator(A, side="right"))
    print("iterations: plain %d, ILU(0) left %d, SPAI right %d" % (plain.iter, left.iter, right.iter))
    for sol in (plain, left, right):
        assert sol.resnorms[-1] <= bc.TOL
    assert left.iter < plain.iter and right.iter < plain.iter
    assert bc.relres(A, right.xk, b) <= bc.TOL * (1 + 1e-6)      # (a right preconditioner leaves the residual's norm alone)
    assert bc.relres(A, plain.xk, b) <= bc.TOL * (1 + 1e-6)
    # from the left the solver's residual is Ml (b - A x): the same quantity in NumPy, through the operator's own dot
    Ml = left.linear_system.Ml
    x = left.xk.reshape(-1, 1)
    res = np.linalg.norm(Ml.dot(b.reshape(-1, 1) - A.dot(x))) / np.linalg.norm(Ml.dot(b.reshape(-1, 1)))
    assert res <= bc.TOL * (1 + 1e-6)
    expect_kernel(hip.get("n_bicgstab_steps") == c0, "operators that are no plain matrix take the generic path")


def test_refusals(hip):
    bc.case_refusals()


def test_convenience(hip):
    bc.case_convenience()
