"""CPU tests of the host side of the one-launch COMPLEX Householder Arnoldi step (``Arnoldi._advance_house`` with a context
that offers ``zhouse_step``), and of the comparison helper the GPU tests use (``tests/support/zhouse_ref.py``).

The NumPy test double has no ``zhouse_step`` and keeps running the per-reflector path.  The context below adds one that
restates the fused step of ``krypy_amd/csrc/house.h`` (``k_zhouse_chain``) in NumPy complex128, from the formulas and not
from the package's code:

* forward links ``d = conj(u_j) . w``, ``w -= (beta_j d) u_j`` for ``j = 0 .. k``, WITHOUT the factors ``conj(alpha_j)``,
  links with ``beta_j == 0`` skipped, ``beta`` a REAL array;
* the new reflector from ``gamma = w[k+1]`` (complex) and ``sigma = ||w[k+2:]||`` with the branches of the reference
  (``krypy/utils.py:349-377``): ``v0 = gamma + gamma / |gamma| xnorm``, ``alpha = -gamma / |gamma|``;
* ``v_{k+1} = alpha_{k+1} H_0 ... H_{k+1} e_{k+1}`` by a descending pass whose first link has the coefficient
  ``beta conj(u_{k+1}[k+1])``;
* returned: a complex array of the raw rows ``0 .. k``, then ``gamma, sigma^2, xnorm, alpha_{k+1}, beta_{k+1}``.

The fixture ``tests/golden/zhouse_arnoldi.npz`` was recorded from the unmodified reference (``tools/gen_zhouse_golden.py``).
Without the complex branch ``zhouse_step`` is never called and the tests fail on its call count."""
import numpy as np
import pytest
import scipy.sparse as sp

from krypy_amd import _hip, utils
from tests.conftest import load_golden
from tests.parity_cases import RTOL
from tests.support.numpy_context import NumpyContext
from tests.support.zhouse_ref import (ZReflectorState, ZStep, assert_zstep_matches, zhouse_step_longdouble, zstep_bars,
                                      zstep_errors)
from tests.support.zhouse_ref import crel as rel          # (complex-aware: parity_cases.rel keeps the real parts only)

DEFECTS = ("dot_without_conj", "e_link_without_conj", "coefficient_re_im_swapped", "sigma2_with_row_k1", "alpha_sign",
           "v_without_alpha")


def zstep_numpy(U, beta, w, k, defect=None):
    """The fused complex step in complex128 (module docstring).  ``defect``: one seeded mistake (``DEFECTS``) - what the
    comparison helper must reject.  Returns ``(out, u, v, beta_new)``."""
    N = w.shape[0]
    w = np.array(w, dtype=np.complex128)

    def link(x, j):
        u = U[:, j]
        d = np.dot(u, x) if defect == "dot_without_conj" else np.vdot(u, x)
        c = beta[j] * d
        if defect == "coefficient_re_im_swapped":
            c = complex(c.imag, c.real)
        return x - c * u

    for j in range(k + 1):
        if beta[j] != 0:
            w = link(w, j)
    gamma = complex(w[k + 1])
    tail = w[k + 2:] if defect != "sigma2_with_row_k1" else w[k + 1:]
    sigma2 = float(np.vdot(tail, tail).real)
    sigma = np.sqrt(sigma2)
    if sigma == 0:
        v0, xnorm, b = 1.0, abs(gamma), 0.0
        alpha = 1.0 if gamma == 0 else gamma / abs(gamma)
    else:
        xnorm, b = np.sqrt(abs(gamma) ** 2 + sigma2), 2.0
        if gamma == 0:
            v0, alpha = -sigma, 1.0
        else:
            v0, alpha = gamma + gamma / abs(gamma) * xnorm, -gamma / abs(gamma)
    if defect == "alpha_sign":
        alpha = -alpha
    s = 1.0 / np.sqrt(abs(v0) ** 2 + sigma2)
    u = np.zeros(N, dtype=np.complex128)
    u[k + 1] = v0 * s
    u[k + 2:] = w[k + 2:] * s
    x = np.zeros(N, dtype=np.complex128)
    x[k + 1] = 1.0
    x -= (b * (u[k + 1] if defect == "e_link_without_conj" else np.conj(u[k + 1]))) * u
    for j in range(k, -1, -1):
        if beta[j] != 0:
            x = link(x, j)
    v = x if defect == "v_without_alpha" else alpha * x
    out = np.concatenate([w[: k + 1], [gamma, sigma2, xnorm, alpha, b]]).astype(np.complex128)
    return out, u, v, b


class ZHouseContext(NumpyContext):
    """The test double plus ``zhouse_step``.  ``serve(k)`` says whether step ``k`` is taken (default: all);
    ``fault_at``: that step reports a timed-out sum once and leaves garbage in what it wrote."""

    def __init__(self, serve=None, fault_at=None):
        NumpyContext.__init__(self)
        self._serve = serve if serve is not None else (lambda k: True)
        self._fault_at = fault_at
        self.served, self.declined, self.faulted = [], [], []

    def zhouse_step(self, Hv, Beta, V, W, wcol, k, slot=0):
        self._count("zhouse_step")
        assert Hv.dtype.kind == V.dtype.kind == W.dtype.kind == "c" and Beta.dtype.kind == "f", "dtypes of a complex step"
        if k + 1 >= V.n or not self._serve(k):
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
        out, u, v, b = zstep_numpy(U, beta, W.a[:, wcol], k)
        U[:, k + 1], V.a[:, k + 1], beta[k + 1] = u, v, b
        self.served.append(k)
        return out


@pytest.fixture
def zhouse_ctx():
    made = []

    def install(**kw):
        ctx = ZHouseContext(**kw)
        old = _hip._install_context_for_testing(ctx)
        if not made:
            made.append(old)
        return ctx

    yield install
    if made:
        _hip._install_context_for_testing(made[0])


def _case(tag):
    g = load_golden("zhouse_arnoldi")
    v = g[tag + "_v"]
    n = v.shape[0]
    A = sp.csr_matrix((g[tag + "_data"], g[tag + "_indices"], g[tag + "_indptr"]), shape=(n, n))
    return A, v, int(g[tag + "_steps"]), g[tag + "_H"], (g[tag + "_Vcols"], g[tag + "_V"])


def _arnoldi(A, v, steps):
    ar = utils.Arnoldi(A, v, maxiter=steps, ortho="house")
    for _ in range(steps):
        ar.advance()
    return ar


def _check(ar, H, V):
    """``V``: the recorded columns of the basis and their indices (all of case a, every fifth of case b)."""
    cols, Vref = V
    assert rel(ar.H, H) < RTOL, rel(ar.H, H)
    assert rel(ar.V[:, cols], Vref) < RTOL, rel(ar.V[:, cols], Vref)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_the_fused_branch_reproduces_the_reference(zhouse_ctx, tag):
    ctx = zhouse_ctx()
    A, v, steps, H, V = _case(tag)
    ar = _arnoldi(A, v, steps)
    # called once per served step (without the complex branch: never), and no reflector is applied on the other path
    assert ctx.calls.get("zhouse_step", 0) == steps
    assert ctx.served == list(range(steps)) and not ctx.declined
    assert ctx.calls.get("dot_panel", 0) == 0 and ctx.calls.get("axpy_panel", 0) == 0
    _check(ar, H, V)
    print("case %s: rel(H) = %.2e, rel(V) = %.2e" % (tag, rel(ar.H, H), rel(ar.V[:, V[0]], V[1])))
    assert ar.H.dtype.kind == "c" and np.all(np.diag(ar.H, -1).imag == 0) and np.all(np.diag(ar.H, -1).real >= 0)
    assert len(ar.houses) == steps + 1 and [h.j for h in ar.houses] == list(range(steps + 1))
    assert all(h.beta in (0, 2) and abs(abs(h.alpha) - 1) < 4e-16 for h in ar.houses)
    assert np.array_equal([h.xnorm for h in ar.houses[1:]], np.diag(ar.H, -1).real)


def test_the_fused_reflector_keeps_a_complex_alpha(zhouse_ctx):
    zhouse_ctx()
    A, v, steps, _, _ = _case("a")
    ar = _arnoldi(A, v, 4)
    for h in ar.houses[1:]:
        assert isinstance(h, utils._FusedHouse) and isinstance(h.alpha, complex) and h.alpha.imag != 0
        assert isinstance(h.beta, float) and isinstance(h.xnorm, float)
    # (and the real step keeps a float)
    assert isinstance(utils._FusedHouse(None, None, 1, np.float64(-1.0), 2.0, 3.0).alpha, float)


def test_the_beta_array_of_a_complex_basis_is_real(zhouse_ctx):
    zhouse_ctx()
    A, v, steps, _, _ = _case("a")
    ar = utils.Arnoldi(A, v, maxiter=steps, ortho="house")
    assert ar._Hbeta is not None and ar._Hbeta.dtype.kind == "f" and ar._Hv.dtype.kind == "c"


def test_declined_steps_take_the_per_reflector_path(zhouse_ctx):
    ctx = zhouse_ctx(serve=lambda k: False)
    A, v, steps, H, V = _case("a")
    ar = _arnoldi(A, v, steps)
    assert ctx.declined == list(range(steps)) and not ctx.served
    assert ctx.calls.get("dot_panel", 0) > 0
    _check(ar, H, V)


def test_both_paths_alternate_on_one_arnoldi_object(zhouse_ctx):
    # steps 0-3 fused, 4-5 per reflector, 6-11 fused: each path applies the other's reflectors and beta entries
    ctx = zhouse_ctx(serve=lambda k: k not in (4, 5))
    A, v, steps, H, V = _case("a")
    ar = _arnoldi(A, v, steps)
    assert ctx.declined == [4, 5] and ctx.served == [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]
    _check(ar, H, V)
    assert [type(h) is utils._FusedHouse for h in ar.houses] == [k not in (0, 5, 6) for k in range(13)]


def test_timed_out_step_is_rerun_and_overwrites_the_garbage(zhouse_ctx):
    ctx = zhouse_ctx(fault_at=5)
    A, v, steps, H, V = _case("a")
    ar = _arnoldi(A, v, steps)
    assert ctx.faulted == [5] and ctx.served == [k for k in range(steps) if k != 5]
    assert np.all(np.isfinite(ar.V)) and np.all(np.isfinite(ar.H))
    assert np.all(np.isfinite(ar._Hv.a[:, : steps + 1])) and np.all(np.isfinite(ar._Hbeta.a[: steps + 1, 0]))
    _check(ar, H, V)


def test_invariant_subspace_agrees_with_the_per_reflector_path(zhouse_ctx, cpu_double):
    N = 50
    A = sp.diags(np.arange(1.0, N + 1) * (1 + 0.25j)).tocsr()
    v = np.zeros((N, 1), dtype=complex)
    v[[3, 17, 41], 0] = [1.0 + 1j, -2.0, 0.5j]

    def run():
        ar = utils.Arnoldi(A, v, maxiter=10, ortho="house")
        while not ar.invariant and ar.iter < 10:
            ar.advance()
        return ar

    old = run()                       # cpu_double: the plain test double, per-reflector path
    ctx = zhouse_ctx()
    new = run()
    assert ctx.served == [0, 1, 2]
    assert old.invariant and new.invariant and old.iter == new.iter == 3
    assert rel(new.H, old.H) < RTOL
    assert rel(new.V[:, :3], old.V[:, :3]) < RTOL
    assert not np.any(new.V[:, 3]) and not np.any(old.V[:, 3])          # the zeroed column
    with pytest.raises(utils.ArgumentError):
        new.advance()


# ---- the comparison helper of the GPU tests ----
def _helper_case(n=97, k=7, seed=5):
    st = ZReflectorState(n, k + 1, seed, zero_beta=(2,))
    rng = np.random.default_rng(seed + 1)
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    U = st.block(0, k + 1)
    ref = zhouse_step_longdouble(st.column, st.beta, w, k)
    yard = zhouse_step_longdouble(st.column, st.beta, w, k, dtype=np.complex128)
    return U, st.beta, w, k, ref, yard


def _as_zstep(res, k):
    out, u, v, _ = res
    return ZStep(out[: k + 1], out[k + 1], out[k + 2], out[k + 3], out[k + 4], out[k + 5], u, v)


def test_the_helper_accepts_the_restated_step():
    U, beta, w, k, ref, yard = _helper_case()
    assert ref.raw.dtype == np.clongdouble and np.finfo(np.longdouble).eps < 2e-19, "no extended precision on this host"
    errs, bars = assert_zstep_matches(_as_zstep(zstep_numpy(U, beta, w, k), k), ref, yard, k, np.linalg.norm(w))
    # nothing in the bar comes from the run under test: the yardstick's own errors and the floor
    _, e64 = zstep_bars(ref, yard, k, np.linalg.norm(w))
    assert all(bars[q] == 16 * max(e64[q], 2.2e-16 * 3.0) for q in bars)
    assert set(errs) == {"raw", "gamma", "sigma2", "xnorm", "alpha", "u", "v"}


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_helper_rejects_a_seeded_defect(defect):
    U, beta, w, k, ref, yard = _helper_case()
    bad = _as_zstep(zstep_numpy(U, beta, w, k, defect=defect), k)
    with pytest.raises(AssertionError):
        assert_zstep_matches(bad, ref, yard, k, np.linalg.norm(w))
    errs = zstep_errors(bad, ref, np.linalg.norm(w))
    print(defect, {q: "%.1e" % e for q, e in errs.items()})


def test_the_helper_rejects_a_nonzero_head_and_a_negative_zero():
    U, beta, w, k, ref, yard = _helper_case()
    out, u, v, _ = zstep_numpy(U, beta, w, k)
    for word in (1e-300, -0.0):
        u2 = u.copy()
        u2[3] = complex(0.0, word)
        with pytest.raises(AssertionError):
            assert_zstep_matches(_as_zstep((out, u2, v, None), k), ref, yard, k, np.linalg.norm(w))
