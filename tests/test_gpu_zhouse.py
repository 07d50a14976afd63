"""GPU tests of the public path of the one-launch complex Householder step (``k_zhouse_chain``, krypy_amd/csrc/house.h;
``Context.zhouse_step``; ``Arnoldi`` / ``Gmres`` with ``ortho='house'`` on complex data).

* the two cases of ``tests/golden/zhouse_arnoldi.npz`` (recorded from the unmodified reference) on the device, ``RTOL``;
* 130 steps on a complex shifted five-point operator of 70,001 rows (35 workgroups): eleven steps are compared step-locally
  with the extended-precision step of ``tests/support/zhouse_ref.py`` fed the state downloaded before the step (its bar:
  ``16 x max(E64, eps sqrt(k + 2))``, nothing from the device), and ``||I - V^H V||_2`` of the basis is held against the
  reference's bound ``k^1.5 N eps`` and within 4 x the per-reflector path's;
* a 40-step complex GMRES at 250,000 rows: its final residual recomputed in NumPy, its H against the same solve with
  ``house_chain = 0`` (``RTOL``)."""
import numpy as np
import pytest
import scipy.sparse as sp

from krypy_amd import linsys, utils
from tests.conftest import load_golden
from tests.parity_cases import RTOL
from tests.support.kernel_expect import expect_kernel
from tests.support.zhouse_ref import ZStep, assert_zstep_matches, crel, zhouse_step_longdouble
from tests.test_gpu_house import SERVED, _per_reflector

pytestmark = pytest.mark.gpu

QS = ("raw", "gamma", "sigma2", "xnorm", "alpha", "u", "v")


def _counts(ctx):
    return ctx.get("n_zhouse_chain"), ctx.get("n_house_recovered"), ctx.get("n_house_chain")


def _run(A, v, steps):
    ar = utils.Arnoldi(A, v.reshape(-1, 1), maxiter=steps, ortho="house")
    while ar.iter < steps and not ar.invariant:
        ar.advance()
    return ar


def _shifted_five_point(n, nx, shift):
    """The five-point stencil on a strip ``nx`` wide, cut off at ``n`` rows (the sizes of the shape classes are no grids),
    minus a complex shift: a Helmholtz-type operator with damping."""
    return sp.diags([-1.0, -1.0, 4.0 - shift, -1.0, -1.0], [-nx, -1, 0, 1, nx], shape=(n, n), dtype=np.complex128).tocsr()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_cases_run_through_the_kernel(hip, tag):
    g = load_golden("zhouse_arnoldi")
    v, steps = g[tag + "_v"], int(g[tag + "_steps"])
    n = v.shape[0]
    A = sp.csr_matrix((g[tag + "_data"], g[tag + "_indices"], g[tag + "_indptr"]), shape=(n, n))
    c0 = _counts(hip)
    ar = _run(A, v, steps)
    c1 = _counts(hip)
    Vgot = ar.V[:, g[tag + "_Vcols"]]          # (the fixture keeps all columns of case a, every fifth of case b)
    print("case %s: rel(H) = %.2e, rel(V) = %.2e" % (tag, crel(ar.H, g[tag + "_H"]), crel(Vgot, g[tag + "_V"])))
    assert crel(ar.H, g[tag + "_H"]) < RTOL and crel(Vgot, g[tag + "_V"]) < RTOL
    assert all(isinstance(h.alpha, complex) for h in ar.houses[1:]) or not SERVED
    assert c1[1] == c0[1] and c1[2] == c0[2]
    expect_kernel(c1[0] - c0[0] == (steps if SERVED else 0), "k_zhouse_chain launches: %d for %d steps" % (c1[0] - c0[0], steps))


def _spy_on_steps(hip, checked, seen):
    """Wrap ``hip.zhouse_step``: the steps in ``checked`` are compared with the reference fed the state downloaded before the
    step.  Returns the function that takes the wrapper off again."""
    inner = hip.zhouse_step

    def spy(Hv, Beta, V, W, wcol, k, slot=0):
        if k not in checked or not SERVED:
            return inner(Hv, Beta, V, W, wcol, k, slot)
        U = Hv.download(0, k + 1)
        beta = Beta.download()[: k + 1, 0]
        w = W.download(wcol, 1)[:, 0]
        out = inner(Hv, Beta, V, W, wcol, k, slot)
        assert out is not None and out is not False, "step %d: %r" % (k, out)
        cols = lambda j: U[:, j]            # noqa: E731
        ref = zhouse_step_longdouble(cols, beta, w, k)
        yard = zhouse_step_longdouble(cols, beta, w, k, dtype=np.complex128)
        wnorm = float(np.linalg.norm(w))
        assert abs(complex(ref.gamma)) >= 1e-6 * wnorm
        got = ZStep(out[: k + 1], out[k + 1], out[k + 2], out[k + 3], out[k + 4], out[k + 5], Hv.download(k + 1, 1)[:, 0],
                    V.download(k + 1, 1)[:, 0])
        errs, bars = assert_zstep_matches(got, ref, yard, k, wnorm)
        print("Arnoldi n = %d, step %d: " % (V.n, k) + ", ".join("%s %.1e/%.1e" % (q, errs[q], bars[q]) for q in QS))
        assert Beta.get(0, k + 1, 1)[0] == float(ref.beta)
        seen.append(k)
        return out

    hip.zhouse_step = spy

    def undo():
        del hip.zhouse_step

    return undo


def test_arnoldi_130_steps_on_a_shifted_laplacian(hip):
    n, steps = 70001, 130
    A = _shifted_five_point(n, 265, 0.5 + 0.75j)
    rng = np.random.default_rng(41)
    v = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    checked = [0, 1, 7, 31, 62, 63, 64, 96, 127, 128, 129]
    seen = []
    c0 = _counts(hip)
    undo = _spy_on_steps(hip, set(checked), seen)
    try:
        ar = _run(A, v, steps)
    finally:
        undo()
    c1 = _counts(hip)
    assert ar.iter == steps and not ar.invariant
    assert seen == (checked if SERVED else [])
    V, H = ar.get()
    eps = np.finfo(float).eps
    orth = np.linalg.norm(np.eye(steps + 1) - V.conj().T.dot(V), 2)
    resid = np.linalg.norm(A.dot(V[:, :steps]) - V.dot(H))
    assert np.count_nonzero(np.tril(H, -2)) == 0 and np.all(np.diag(H, -1).imag == 0) and np.all(np.diag(H, -1).real >= 0)
    with _per_reflector(hip):
        old = _run(A, v, 40)
    Vo, Ho = old.get()
    o_new = np.linalg.norm(np.eye(41) - V[:, :41].conj().T.dot(V[:, :41]), 2)
    o_old = np.linalg.norm(np.eye(41) - Vo.conj().T.dot(Vo), 2)
    print("n = %d: ||I - V^H V||_2 = %.3e over %d columns (bound %.3e), %.3e over the first 41 (per-reflector run: %.3e); "
          "||A V_k - V_{k+1} H|| = %.3e" % (n, orth, steps + 1, steps ** 1.5 * n * eps, o_new, o_old, resid))
    assert orth <= steps ** 1.5 * n * eps          # (the reference's own test bound)
    assert resid <= 8 * steps * n ** 1.5 * eps
    assert o_new <= 4 * o_old, (o_new, o_old)
    assert crel(H[:41, :40], Ho) < RTOL and crel(V[:, :41], Vo) < RTOL
    assert c1[1] == c0[1] and c1[2] == c0[2], "a launch reported a timed-out sum, or the real counter moved"
    expect_kernel(c1[0] - c0[0] == (steps if SERVED else 0), "k_zhouse_chain launches in %d steps: %d" % (steps, c1[0] - c0[0]))


def test_gmres_house_250k_complex(hip):
    nx = 500
    n = nx * nx
    A = _shifted_five_point(n, nx, -(0.5 + 1.0j))          # (4.5 + i on the diagonal: 40 steps gain several digits)
    rng = np.random.default_rng(42)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    b = (b / np.linalg.norm(b)).reshape(-1, 1)

    def solve():
        try:
            return linsys.Gmres(linsys.LinearSystem(A, b), ortho="house", tol=1e-30, maxiter=40)
        except utils.ConvergenceError as e:
            return e.solver

    c0 = _counts(hip)
    s = solve()
    c1 = _counts(hip)
    with _per_reflector(hip):
        old = solve()
    c2 = _counts(hip)
    assert s.arnoldi.iter == 40 == old.arnoldi.iter
    x = np.asarray(s.xk[:, 0])
    final = float(np.linalg.norm(b[:, 0] - A.dot(x)) / np.linalg.norm(b[:, 0]))
    print("GMRES(house) at n = %d, 40 steps: last residual norm of the recurrence %.6e, recomputed %.6e; against "
          "house_chain = 0: rel(H) = %.2e, rel(x) = %.2e" % (n, s.resnorms[-1], final, crel(s.arnoldi.H, old.arnoldi.H),
                                                            crel(s.xk, old.xk)))
    assert final < 1e-3, "40 steps must have gained three digits on this operator"
    # the recurrence and the recomputed residual differ by rounding of O(eps ||A|| ||x||) ~ 1e-15 absolutely, 1e-4 of a
    # residual of 7e-12: held to one percent of the recurrence's figure
    assert abs(final - s.resnorms[-1]) <= 1e-2 * s.resnorms[-1]
    assert crel(s.arnoldi.H, old.arnoldi.H) < RTOL and crel(s.xk, old.xk) < RTOL
    assert c2 == c1, "house_chain = 0 still launched the kernel"
    assert c1[1] == c0[1] and c1[2] == c0[2]
    expect_kernel(c1[0] - c0[0] == (40 if SERVED else 0), "k_zhouse_chain launches: %d for 40 Arnoldi steps" % (c1[0] - c0[0]))
