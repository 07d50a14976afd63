"""CPU tests of the host side of the one-launch Householder Arnoldi step (``Arnoldi._advance_house`` with a context that
offers ``house_step``).

The NumPy test double has no ``house_step`` and keeps running the per-reflector path.  The context below adds one that
restates the fused step of ``krypy_amd/csrc/house.h`` in NumPy, from the formulas and not from the package's code:

* forward links ``d = <u_j, w>``, ``w -= (beta_j d) u_j`` for ``j = 0 .. k``, WITHOUT the factors ``conj(alpha_j)``,
  links with ``beta_j == 0`` skipped;
* the new reflector from ``gamma = w[k+1]`` and ``sigma = ||w[k+2:]||`` with the branches and signs of the reference
  (``krypy/utils.py:349-377``), written to column ``k+1`` of the reflector block, ``beta_{k+1}`` to the beta array;
* ``v_{k+1} = alpha_{k+1} H_0 ... H_{k+1} e_{k+1}`` by a descending pass;
* returned: the raw rows ``0 .. k``, then ``gamma, sigma^2, xnorm, alpha_{k+1}, beta_{k+1}``.

What is tested is the Python branch: the H column it assembles (``raw * conj(alpha)``, ``H[k+1, k] = xnorm``), the
reflector objects it appends, the declined-step and timed-out-step fallbacks, the alternation of both paths on one
Arnoldi object, and the invariance bookkeeping - against the fixture recorded from the reference.  Without the branch
``house_step`` is never called and the tests here fail on its call count - all but the last one, a guard that complex
data never reaches the fused step, which holds with or without the branch."""
import numpy as np
import pytest
import scipy.sparse as sp

from krypy_amd import _hip, linsys, utils
from oracle.inputs import lap2d_system
from tests.conftest import load_golden
from tests.parity_cases import RTOL, check_resnorms, rel
from tests.support.numpy_context import NumpyContext


class HouseContext(NumpyContext):
    """The test double plus ``house_step``.  ``serve(k)`` says whether step ``k`` is taken (default: all);
    ``fault_at``: that step reports a timed-out sum once and leaves garbage in what it wrote."""

    def __init__(self, serve=None, fault_at=None):
        NumpyContext.__init__(self)
        self._serve = serve if serve is not None else (lambda k: True)
        self._fault_at = fault_at
        self.served, self.declined, self.faulted = [], [], []

    def house_step(self, Hv, Beta, V, W, wcol, k, slot=0):
        self._count("house_step")
        N = V.n
        if Hv.dtype.kind == "c" or k + 1 >= N or not self._serve(k):
            self.declined.append(k)
            return None
        U, beta = Hv.a, Beta.a[:, 0]
        if self._fault_at == k:
            self._fault_at = None
            self.faulted.append(k)
            U[:, k + 1] = np.nan
            V.a[:, k + 1] = np.nan
            beta[k + 1] = np.nan
            return False
        w = W.a[:, wcol].copy()
        for j in range(k + 1):
            if beta[j] != 0:
                w -= (beta[j] * np.dot(U[:, j], w)) * U[:, j]
        gamma = w[k + 1]
        sigma2 = float(np.dot(w[k + 2:], w[k + 2:]))
        sigma = np.sqrt(sigma2)
        if sigma == 0:
            v0, xnorm, b = 1.0, abs(gamma), 0.0
            alpha = 1.0 if gamma == 0 else gamma / abs(gamma)
        else:
            xnorm, b = np.sqrt(gamma * gamma + sigma * sigma), 2.0
            if gamma == 0:
                v0, alpha = -sigma, 1.0
            else:
                v0, alpha = gamma + np.sign(gamma) * xnorm, -np.sign(gamma)
        s = 1.0 / np.sqrt(v0 * v0 + sigma * sigma)
        u = np.zeros(N)
        u[k + 1] = v0 * s
        u[k + 2:] = w[k + 2:] * s
        U[:, k + 1] = u
        beta[k + 1] = b
        x = np.zeros(N)
        x[k + 1] = 1.0
        x -= (b * u[k + 1]) * u
        for j in range(k, -1, -1):
            if beta[j] != 0:
                x -= (beta[j] * np.dot(U[:, j], x)) * U[:, j]
        V.a[:, k + 1] = alpha * x
        self.served.append(k)
        return np.concatenate([w[: k + 1], [gamma, sigma2, xnorm, alpha, b]])


@pytest.fixture
def house_ctx():
    made = []

    def install(**kw):
        ctx = HouseContext(**kw)
        if not made:
            made.append(_hip._install_context_for_testing(ctx))
        else:
            _hip._install_context_for_testing(ctx)
        return ctx

    yield install
    if made:
        _hip._install_context_for_testing(made[0])


def _fixture_case():
    A, b = lap2d_system(40, rhs="rng1")
    return A, b, load_golden("kernels")


def _arnoldi(A, v, steps, **kw):
    ar = utils.Arnoldi(A, v, maxiter=steps, ortho="house", **kw)
    for _ in range(steps):
        ar.advance()
    return ar


def _check_reference_inequalities(A, ar, k):
    V, H = ar.get()
    N = A.shape[0]
    eps = np.finfo(float).eps
    assert np.linalg.norm(np.eye(k + 1) - V.T.dot(V), 2) <= (k ** 1.5) * N * eps
    assert np.all(np.diag(H, -1) >= 0) and np.linalg.norm(np.tril(H, -2)) == 0
    assert np.linalg.norm(A.dot(V[:, :k]) - V.dot(H)) <= k * N ** 1.5 * eps * 8


def test_arnoldi_house_through_the_fused_branch(house_ctx):
    ctx = house_ctx()
    A, b, g = _fixture_case()
    ar = _arnoldi(A, b.reshape(-1, 1), 12)
    assert ctx.served == list(range(12)) and not ctx.declined
    # (the per-reflector path was not used for any step: one dot_panel per reflector application would show here)
    assert ctx.calls.get("dot_panel", 0) == 0 and ctx.calls.get("axpy_panel", 0) == 0
    assert rel(ar.H, g["arn_house_H"]) < RTOL
    assert rel(ar.V, g["arn_house_V"]) < RTOL
    _check_reference_inequalities(A, ar, 12)
    # the reflector objects: one per column, scalars as the step reported them, usable by the other path
    assert len(ar.houses) == 13 and [h.j for h in ar.houses] == list(range(13))
    assert all(h.beta in (0, 2) and abs(h.alpha) == 1 for h in ar.houses)
    assert np.allclose([h.xnorm for h in ar.houses[1:]], np.diag(ar.H, -1), rtol=0, atol=0)


def test_gmres_house_through_the_fused_branch(house_ctx):
    ctx = house_ctx()
    A, b, g = _fixture_case()
    s = linsys.Gmres(linsys.LinearSystem(A, b), ortho="house", tol=1e-9, maxiter=200)
    assert len(ctx.served) == s.arnoldi.iter >= s.iter and not ctx.declined
    check_resnorms(s.resnorms, g["gmres_house_resnorms"], tol=1e-8, explicit_tol=1e-4)
    assert rel(s.xk[:, 0], g["gmres_house_xk"]) < 1e-9


def test_declined_steps_take_the_per_reflector_path(house_ctx):
    ctx = house_ctx(serve=lambda k: False)
    A, b, g = _fixture_case()
    ar = _arnoldi(A, b.reshape(-1, 1), 12)
    assert ctx.declined == list(range(12)) and not ctx.served
    assert ctx.calls.get("dot_panel", 0) > 0
    assert rel(ar.H, g["arn_house_H"]) < RTOL and rel(ar.V, g["arn_house_V"]) < RTOL


def test_both_paths_alternate_on_one_arnoldi_object(house_ctx):
    # steps 0-3 fused, 4-5 per reflector, 6-11 fused: each path applies the other's reflectors and beta entries
    ctx = house_ctx(serve=lambda k: k not in (4, 5))
    A, b, g = _fixture_case()
    ar = _arnoldi(A, b.reshape(-1, 1), 12)
    assert ctx.declined == [4, 5] and ctx.served == [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]
    assert rel(ar.H, g["arn_house_H"]) < RTOL and rel(ar.V, g["arn_house_V"]) < RTOL
    _check_reference_inequalities(A, ar, 12)


def test_timed_out_step_is_rerun_from_the_untouched_product(house_ctx):
    ctx = house_ctx(fault_at=5)
    A, b, g = _fixture_case()
    ar = _arnoldi(A, b.reshape(-1, 1), 12)
    assert ctx.faulted == [5] and ctx.served == [k for k in range(12) if k != 5]
    assert np.all(np.isfinite(ar.V)) and np.all(np.isfinite(ar.H))
    assert rel(ar.H, g["arn_house_H"]) < RTOL and rel(ar.V, g["arn_house_V"]) < RTOL


def test_invariant_subspace_agrees_with_the_per_reflector_path(house_ctx, cpu_double):
    N = 50
    A = sp.diags(np.arange(1.0, N + 1)).tocsr()
    v = np.zeros((N, 1))
    v[[3, 17, 41], 0] = [1.0, -2.0, 0.5]

    def run():
        ar = utils.Arnoldi(A, v, maxiter=10, ortho="house")
        while not ar.invariant and ar.iter < 10:
            ar.advance()
        return ar

    old = run()                       # cpu_double: the plain test double, per-reflector path
    ctx = house_ctx()
    new = run()
    assert ctx.served == [0, 1, 2]
    assert old.invariant and new.invariant and old.iter == new.iter == 3
    assert rel(new.H, old.H) < RTOL
    assert rel(new.V[:, :3], old.V[:, :3]) < RTOL
    assert not np.any(new.V[:, 3]) and not np.any(old.V[:, 3])          # the zeroed column
    with pytest.raises(utils.ArgumentError):
        new.advance()


def test_complex_data_never_reaches_the_fused_step(house_ctx):
    ctx = house_ctx()
    A, b, _ = _fixture_case()
    ar = _arnoldi(A.astype(complex), (b * (1 + 0.5j)).reshape(-1, 1), 4)
    assert ctx.calls.get("house_step", 0) == 0          # (no beta array is kept for a complex basis)
    assert np.linalg.norm(np.eye(5) - ar.V.conj().T.dot(ar.V), 2) < 1e-12
