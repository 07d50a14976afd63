"""GPU tests of the one-launch Householder Arnoldi step (``k_house_chain``, krypy_amd/csrc/house.h;
``kh_house_step_begin`` / ``_end``; ``Arnoldi(ortho='house')``).

The per-reflector path (``ctx.set("house_chain", 0)``: one dot, one axpy and a host round trip per reflector - what every
step ran before the kernel existed) is the comparison throughout; the reference's own fixture and inequalities
(``parity_cases.case_arnoldi_house``) hold for both.  Tolerances: the project's ``RTOL = 1e-10`` between the two paths -
two NumPy runs of the 250,000-row case that differ only in summation order move ``H`` by 7.3e-16 and ``V`` by 5.5e-15, so
the bar has five orders of margin and still fails on any wrong link - and a factor 4 on ``||I - V^T V||_2`` (the same two
runs differ by 1.3 x)."""
import contextlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

from krypy_amd import utils
from tests import parity_cases as pc
from tests.parity_cases import RTOL, rel
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal, poisoned_allocations

pytestmark = pytest.mark.gpu

# (robustness runs push the whole suite through the multi-rank code path: the kernel declines a communicator)
SERVED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") != "1"


def _counts(ctx):
    return ctx.get("n_house_chain"), ctx.get("n_house_recovered")


@contextlib.contextmanager
def _per_reflector(ctx):
    ctx.set("house_chain", 0)
    try:
        yield
    finally:
        ctx.set("house_chain", 1)


def _run(A, v, steps, switch=None, ctx=None):
    """``steps`` Householder Arnoldi steps (fewer when the subspace turns out invariant); ``switch(k)`` is called before
    step ``k``."""
    ar = utils.Arnoldi(A, v.reshape(-1, 1), maxiter=steps, ortho="house")
    while ar.iter < steps and not ar.invariant:
        if switch is not None:
            switch(ar.iter)
        ar.advance()
    return ar


def _convection_diffusion(nx):
    """5-point Laplacian plus a first-order convection term on an nx x nx grid: non-symmetric."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    I = sp.identity(nx)
    A = sp.kron(I, T) + sp.kron(T, I) + sp.kron(I, sp.diags([-0.3, 0.3], [-1, 1], shape=(nx, nx)))
    return A.tocsr()


def _banded(n):
    """A non-symmetric banded operator of any size n (the shape-class sizes are no grids)."""
    return sp.diags([-1.3, 2.0, -0.7, 0.25], [-1, 0, 1, 7], shape=(n, n)).tocsr()


def _check_reference_inequalities(A, V, H):
    N, k = A.shape[0], H.shape[1]
    eps = np.finfo(float).eps
    orth = np.linalg.norm(np.eye(k + 1) - V.T.dot(V), 2)
    print("  ||I - V^T V||_2 = %.3e (bound %.3e)" % (orth, (k ** 1.5) * N * eps))
    assert orth <= (k ** 1.5) * N * eps
    resid = np.linalg.norm(A.dot(V[:, :k]) - V.dot(H))
    print("  ||A V_k - V_{k+1} H|| = %.3e (bound %.3e)" % (resid, 8 * k * N ** 1.5 * eps))
    assert resid <= 8 * k * N ** 1.5 * eps
    assert np.all(np.diag(H, -1) >= 0) and np.linalg.norm(np.tril(H, -2)) == 0
    return orth


def _compare_paths(ctx, A, v, steps, served=True):
    """Both paths on the same input: counters, RTOL between them, the reference's inequalities for both, orthogonality
    of the new path within 4 x the old one's.  Returns the fused run."""
    c0 = _counts(ctx)
    new = _run(A, v, steps)
    c1 = _counts(ctx)
    with _per_reflector(ctx):
        old = _run(A, v, steps)
    c2 = _counts(ctx)
    Vn, Hn = new.get()
    Vo, Ho = old.get()
    print("N = %d, %d steps: rel(H) = %.3e, rel(V) = %.3e" % (A.shape[0], steps, rel(Hn, Ho), rel(Vn, Vo)))
    assert rel(Hn, Ho) < RTOL
    assert rel(Vn, Vo) < RTOL
    on = _check_reference_inequalities(A, Vn, Hn)
    oo = _check_reference_inequalities(A, Vo, Ho)
    assert on <= 4 * oo, (on, oo)
    assert c2 == c1, "house_chain = 0 still launched the kernel"
    assert c1[1] == c0[1], "a launch reported a timed-out sum"
    expect_kernel(c1[0] - c0[0] == (steps if served and SERVED else 0),
                  "k_house_chain launches for N = %d: %d, expected %d" % (A.shape[0], c1[0] - c0[0], steps if served and SERVED else 0))
    return new


def test_reference_parity_runs_through_the_kernel(hip):
    """The reference's fixture (lap2d 40 x 40, 12 steps, and GMRES to 1e-9) with every step served by k_house_chain."""
    taken = []
    original = utils.Arnoldi._advance_house

    def counted(self, k):
        taken.append(k)
        return original(self, k)

    c0 = _counts(hip)
    utils.Arnoldi._advance_house = counted
    try:
        pc.case_arnoldi_house()
    finally:
        utils.Arnoldi._advance_house = original
    c1 = _counts(hip)
    assert len(taken) > 12
    assert c1[1] == c0[1]
    assert c1[0] - c0[0] == (len(taken) if SERVED else 0), (c1[0] - c0[0], len(taken))


_big = {}


def _big_case():
    if not _big:
        A = _convection_diffusion(500)
        _big["A"], _big["v"] = A, np.random.default_rng(1).standard_normal(A.shape[0])
    return _big["A"], _big["v"]


def test_fused_against_per_reflector_path_250k(hip):
    A, v = _big_case()
    _big["fused"] = _compare_paths(hip, A, v, 60)


@pytest.mark.parametrize("n", [3001,          # a short vector in an unpadded block: the MASKED kernel, 4 rows per lane
                               1000003,       # 4 rows per lane, odd length, a partial last workgroup
                               1100001,       # 8 rows per lane
                               2200000,       # 16
                               4300000,       # 24
                               6400000,       # 32
                               10000000])     # 40: the largest served shape
def test_every_shape_class(hip, n):
    A = _banded(n)
    v = np.random.default_rng(n).standard_normal(n)
    _compare_paths(hip, A, v, 8)


def test_beyond_the_served_range_takes_the_old_path(hip):
    """More than 40 double2 rows per lane on 256 compute units: declined, nothing launched, results still right."""
    n = 10600000
    if hip.info()["compute_units"] * 40 * 512 * 2 >= n:
        n = hip.info()["compute_units"] * 40 * 512 * 2 + 100001
    A = _banded(n)
    v = np.random.default_rng(5).standard_normal(n)
    c0 = _counts(hip)
    ar = _run(A, v, 4)
    assert _counts(hip) == c0
    V, H = ar.get()
    _check_reference_inequalities(A, V, H)


def test_invariant_subspace(hip):
    n = 20000
    A = sp.diags(np.arange(1.0, n + 1)).tocsr()
    v = np.zeros(n)
    v[[3, 1700, 15001]] = [1.0, -2.0, 0.5]
    c0 = _counts(hip)
    new = _run(A, v, 10)
    c1 = _counts(hip)
    with _per_reflector(hip):
        old = _run(A, v, 10)
    assert new.invariant and old.invariant and new.iter == old.iter == 3
    assert rel(new.H, old.H) < RTOL
    assert rel(new.V[:, :3], old.V[:, :3]) < RTOL
    assert not np.any(new.V[:, 3]) and not np.any(old.V[:, 3])
    expect_kernel(c1[0] - c0[0] == (3 if SERVED else 0), "k_house_chain launches: %d, expected 3" % (c1[0] - c0[0]))


@pytest.mark.parametrize("n", [5001, 300001])
def test_exact_breakdown_writes_nothing_non_finite(hip, n):
    """w[k+1:] exactly zero (sigma == gamma == 0): A diagonal, v = e_0.  The new reflector is e_1 with beta = 0, H[1, 0] = 0,
    and no 0 / 0 reaches the reflector block, the basis or their padding."""
    A = sp.diags(np.linspace(2.0, 3.0, n)).tocsr()
    v = np.zeros(n)
    v[0] = 1.5
    c0 = _counts(hip)
    ar = utils.Arnoldi(A, v.reshape(-1, 1), maxiter=6, ortho="house")
    ar.advance()
    c1 = _counts(hip)
    assert ar.invariant and ar.iter == 1
    assert ar.H[0, 0] == 2.0 and ar.H[1, 0] == 0.0
    Hv = ar._Hv.download()
    assert np.all(np.isfinite(Hv))
    assert np.all(np.isfinite(ar._V.download(0, 2)))
    e1 = np.zeros(n)
    e1[1] = 1.0
    if SERVED:
        assert np.array_equal(Hv[:, 1], e1) and ar.houses[1].beta == 0
    assert ar._Hv.padding_nonzero() == 0 and ar._V.padding_nonzero() == 0      # (a NaN counts as non-zero)
    expect_kernel(c1[0] - c0[0] == (1 if SERVED else 0), "k_house_chain launches: %d, expected 1" % (c1[0] - c0[0]))


@pytest.mark.parametrize("n", [3001, 100003])
def test_poisoned_blocks(hip, n):
    """Nothing unwritten is read (the run on blocks full of NaN has the bits of the run on zeroed ones) and the padding
    of the reflector block and of the basis is zero afterwards."""
    A = _banded(n)
    v = np.random.default_rng(7).standard_normal(n)
    clean = _run(A, v, 8)
    Vc, Hc = clean.get()
    c0 = _counts(hip)
    with poisoned_allocations(hip) as rec:
        dirty = _run(A, v, 8)
        Vd, Hd = dirty.get()
        assert rec.poisoned > 0
        bits_equal(Hd, Hc, "H")
        bits_equal(Vd, Vc, "V")
        bits_equal(dirty._Hv.download(0, 9), clean._Hv.download(0, 9), "reflector block")
        assert dirty._Hv.padding_nonzero() == 0 and dirty._V.padding_nonzero() == 0
        assert dirty._Hbeta.padding_nonzero() == 0
    expect_kernel(_counts(hip)[0] - c0[0] == (8 if SERVED else 0), "k_house_chain launches on poisoned blocks")


def test_timed_out_launch_is_recovered_on_the_old_path(hip):
    A = _banded(200000)
    v = np.random.default_rng(3).standard_normal(200000)
    with _per_reflector(hip):
        old = _run(A, v, 8)
    counts = {}

    def switch(k):
        counts[k] = _counts(hip)
        if k == 5:
            hip.set("chain_fault", 1)

    try:
        new = _run(A, v, 8, switch=switch)
        end = _counts(hip)
    finally:
        hip.set("chain_fault", 0)
        hip.set("house_chain", 1)        # (starts the context's count of timeouts again)
    assert rel(new.H[:, 5], old.H[:, 5]) < RTOL and rel(new.V[:, 6], old.V[:, 6]) < RTOL
    assert rel(new.H, old.H) < RTOL and rel(new.V, old.V) < RTOL
    if SERVED:
        assert counts[6][1] - counts[5][1] == 1 and end[1] - counts[0][1] == 1       # one recovery, at step 5
        assert counts[7][0] - counts[6][0] == 1 and end[0] - counts[7][0] == 1       # steps 6 and 7 ran fused again
        assert end[0] - counts[0][0] == 8                                            # (the faulted launch counts as one)


def test_both_paths_alternate_on_one_basis(hip):
    A, v = _big_case()
    fused = _big.get("fused") or _run(A, v, 60)
    c0 = _counts(hip)
    mixed = _run(A, v, 10, switch=lambda k: hip.set("house_chain", 0 if k in (4, 5) else 1))
    hip.set("house_chain", 1)
    c1 = _counts(hip)
    assert rel(mixed.H, fused.H[:11, :10]) < RTOL
    assert rel(mixed.V, fused.V[:, :11]) < RTOL
    expect_kernel(c1[0] - c0[0] == (8 if SERVED else 0), "k_house_chain launches: %d, expected 8 of 10 steps" % (c1[0] - c0[0]))


def test_two_fused_runs_are_bit_identical(hip):
    A, v = _big_case()
    first = _big.get("fused") or _run(A, v, 60)
    second = _run(A, v, 60)
    bits_equal(second.H, first.H, "H")
    bits_equal(second.V, first.V, "V")
