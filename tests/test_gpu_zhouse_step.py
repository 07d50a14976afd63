"""GPU tests of ``k_zhouse_chain`` (krypy_amd/csrc/house.h: the one-launch Householder step for complex data) against an
extended-precision reference written outside the package (``tests/support/zhouse_ref.py``).

``hip.zhouse_step`` is called DIRECTLY on constructed state - seeded unit complex reflector columns, factors 2.0 or 0.0, a
random complex ``w``, NaN in everything the call is to write - so that every boundary of the kernel is reached without
running a thousand Arnoldi steps first: wave boundaries (``k + 1`` = 63, 64), the last lanes of the two register rows the raw
H entries come from (``k`` = 1021, 1022), the decline at ``k + 2 > 1024`` and at ``k + 1 >= n``, every served rows-per-lane
class and the declined one, runs of skipped links, the scalar branches, tiny vectors, the plumbing (``wcol``, slots).

THE BAR (``zhouse_ref.assert_zstep_matches``), for every compared quantity: ``16 x max(E64, eps sqrt(k + 2))``, ``eps = 2.2e-16``.
``E64`` is the error of a complex128 NumPy evaluation of the same step on the same inputs against the extended-precision one,
computed in the test; the factor 16 covers another order of summation.  Neither figure comes from the device.
``raw[0..k]`` and ``gamma``: max-abs error over ``||w||``; ``sigma^2`` and ``xnorm``: relative; ``alpha``: absolute;
``beta_{k+1}``: exact; ``u_{k+1}`` and ``v_{k+1}``: 2-norm of the difference.  The device's own errors are printed per case and
as a table at the end of the module (``ZHOUSE-STEP DEVICE ERRORS``; KERNELS.md 4.20 quotes one run).

With ``KRYPY_AMD_TEST_FORCE_MULTI=1`` the kernel declines: a direct call must return ``None`` and leave every block bit for
bit as it was - that is checked, then the numeric part is skipped (a direct call has no per-reflector form)."""
import time

import numpy as np
import pytest

from krypy_amd import utils
from tests.parity_cases import RTOL
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal
from tests.support.zhouse_ref import ZReflectorState, ZStep, assert_zstep_matches, crel, zhouse_step_longdouble
from tests.test_gpu_house import SERVED

pytestmark = pytest.mark.gpu

C128 = np.complex128
NAN = complex(np.nan, np.nan)          # what the two target columns hold before a call (beta[k+1]: NaN)
LIMIT_K = 1022                         # the last served step: k + 2 <= 1024
NOT_SERVED = "KRYPY_AMD_TEST_FORCE_MULTI=1: zhouse_step declines (checked: None, blocks untouched); a direct call has no " \
             "per-reflector form to run the numeric part on"
QS = ("raw", "gamma", "sigma2", "xnorm", "alpha", "u", "v")

_measured = {}               # (quantity, n) -> (largest device error, its bar, k)


@pytest.fixture(scope="module", autouse=True)
def _report_device_errors():
    t0 = time.time()
    yield
    print("\nZHOUSE-STEP DEVICE ERRORS (largest per quantity and length; bar of that case; k of that case)")
    for n in sorted({key[1] for key in _measured}):
        print("  n = %-9d" % n + "  ".join("%s %.2e / %.2e (k=%d)" % ((q,) + _measured[(q, n)])
                                           for q in QS if (q, n) in _measured))
    print("ZHOUSE-STEP MODULE WALL TIME %.1f s" % (time.time() - t0))


def _record(n, k, errs, bars):
    for q, e in errs.items():
        if (q, n) not in _measured or e > _measured[(q, n)][0]:
            _measured[(q, n)] = (e, bars[q], k)


def _counts(ctx):
    return ctx.get("n_zhouse_chain"), ctx.get("n_house_recovered"), ctx.get("n_house_chain")


def _crandn(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


class _Rig(object):
    """Device blocks for direct calls on a constructed state of ``ncols`` complex reflectors of length ``n``: ``Hv`` and ``V``
    have ``ncols + 3`` columns (step ``k = ncols - 1`` writes column ``ncols``, the sentinel sits behind it; a declined step
    ``k = ncols`` is prepared the same way), ``Beta`` (real) ``ncols + 3`` entries.  Column ``c`` of ``V`` holds
    ``(c + 1) * vfill``.  A host copy of the reflector block is kept up to 2 GB; beyond that columns are made again from
    their seeds."""

    def __init__(self, hip, n, ncols, seed, zero_beta=(), wcols=1):
        self.hip, self.n, self.ncols = hip, n, ncols
        self.state = ZReflectorState(n, ncols, seed, zero_beta)
        self.Hv = hip.alloc(n, ncols + 3, dtype=C128)
        self.V = hip.alloc(n, ncols + 3, dtype=C128)
        self.Beta = hip.alloc(ncols + 3, 1)
        self.W = hip.alloc(n, wcols, dtype=C128)
        self.U = self.state.block(0, ncols) if 16.0 * n * ncols <= 2e9 else None
        rng = np.random.default_rng([seed, 77])
        self.vfill = _crandn(rng, n)
        self.sentinel = _crandn(rng, n)
        for j0 in range(0, ncols, 64):
            j1 = min(ncols, j0 + 64)
            self.Hv.upload(j0, self.U[:, j0:j1] if self.U is not None else self.state.block(j0, j1))
        for c0 in range(0, ncols + 3, 64):
            cs = np.arange(c0, min(ncols + 3, c0 + 64))
            self.V.upload(c0, self.vfill[:, None] * (cs + 1.0)[None, :])
        self.small = float(n) * (ncols + 3) <= 1e7

    def column(self, j):
        return self.U[:, j] if self.U is not None else self.state.column(j)

    def beta_image(self, k):
        b = np.full(self.ncols + 3, 0.125)
        b[: self.ncols] = self.state.beta
        b[k + 1] = np.nan
        return b


def _pick_w(rig, k, seed):
    """A random complex ``w`` and its reference step (``|gamma| >= 1e-6 ||w||``: ``alpha = -gamma / |gamma|`` is then
    determined to far better than the bar; reseeded otherwise)."""
    for attempt in range(6):
        w = _crandn(np.random.default_rng([seed, k, attempt]), rig.n)
        ref = zhouse_step_longdouble(rig.column, rig.state.beta, w, k)
        if abs(complex(ref.gamma)) >= 1e-6 * float(np.linalg.norm(w)):
            return w, ref
    raise AssertionError("no w with |gamma| >= 1e-6 ||w|| in six seeds: n = %d, k = %d" % (rig.n, k))


def _v_column(rig, c):
    return rig.vfill * (c + 1.0)


def _check_untouched(rig, k, wimage, bimage, targets_too):
    """Columns 0 .. k and the sentinel column of Hv, every column of V but k + 1 (a sample of three when the block is large),
    W, Beta but entry k + 1, the padding of all four; ``targets_too``: the call was declined - the target columns and
    beta[k+1] still hold their NaN."""
    have = min(k + 1, rig.ncols)          # (a declined step k = ncols: the state has no column k)
    if rig.U is not None:
        bits_equal(rig.Hv.download(0, have), rig.U[:, :have], "reflector columns 0 .. %d" % (have - 1))
    else:
        for j in range(have):
            bits_equal(rig.Hv.download(j, 1)[:, 0], rig.state.column(j), "reflector column %d" % j)
    bits_equal(rig.Hv.download(k + 2, 1)[:, 0], rig.sentinel, "the column behind the new reflector")
    if rig.small:
        Vd = rig.V.download()
        for c in range(rig.V.ncols):
            if c != k + 1:
                bits_equal(Vd[:, c], _v_column(rig, c), "basis column %d" % c)
    else:
        for c in sorted({0, k, k + 2}):
            bits_equal(rig.V.download(c, 1)[:, 0], _v_column(rig, c), "basis column %d" % c)
    bits_equal(rig.W.download(), wimage, "W")
    b = rig.Beta.download()[:, 0]
    keep = np.arange(b.size) != k + 1
    bits_equal(b[keep], bimage[keep], "beta entries other than k + 1")
    if targets_too:
        junk = np.full(rig.n, NAN)
        bits_equal(rig.Hv.download(k + 1, 1)[:, 0], junk, "reflector column k + 1 of a declined step")
        bits_equal(rig.V.download(k + 1, 1)[:, 0], junk, "basis column k + 1 of a declined step")
        bits_equal(b[k + 1: k + 2], bimage[k + 1: k + 2], "beta[k + 1] of a declined step")
    assert rig.Hv.padding_nonzero() == 0 and rig.V.padding_nonzero() == 0
    assert rig.W.padding_nonzero() == 0 and rig.Beta.padding_nonzero() == 0


def _prepare(rig, k, w, wcol):
    junk = np.full(rig.n, NAN)
    rig.Hv.upload(k + 1, junk)
    rig.Hv.upload(k + 2, rig.sentinel)
    rig.V.upload(k + 1, junk)
    bimage = rig.beta_image(k)
    rig.Beta.upload(0, bimage)
    rig.W.upload(wcol, w)
    return rig.W.download(), bimage


def _restore(rig, k):
    """Put back what a call at step k and its preparation overwrote, so that the next call finds the constructed state."""
    rig.V.upload(k + 1, _v_column(rig, k + 1))
    for c in (k + 1, k + 2):
        if c < rig.ncols:
            rig.Hv.upload(c, rig.column(c))


def _declined(rig, k, w, wcol=0, slot=0):
    """A call the kernel must decline: None, no launch, every block bit for bit as it was."""
    wimage, bimage = _prepare(rig, k, w, wcol)
    c0 = _counts(rig.hip)
    out = rig.hip.zhouse_step(rig.Hv, rig.Beta, rig.V, rig.W, wcol, k, slot)
    assert out is None, "step k = %d at n = %d was not declined" % (k, rig.n)
    assert _counts(rig.hip) == c0
    _check_untouched(rig, k, wimage, bimage, targets_too=True)
    _restore(rig, k)


def _as_zstep(out, u, v, k):
    return ZStep(out[: k + 1], out[k + 1], out[k + 2], out[k + 3], out[k + 4], out[k + 5], u, v)


def _step(rig, k, w, ref=None, wcol=0, slot=0, structure=True):
    """One served call, compared with the reference and checked for what it must not touch.  Returns
    ``(out, u, v, ref)`` - or None when the kernel is switched off for the whole run (FORCE_MULTI)."""
    hip, n = rig.hip, rig.n
    if not SERVED:
        _declined(rig, k, w, wcol, slot)
        return None
    if ref is None:
        ref = zhouse_step_longdouble(rig.column, rig.state.beta, w, k)
    wnorm = float(np.linalg.norm(w))
    assert ref.gamma == 0 or abs(complex(ref.gamma)) >= 1e-6 * wnorm, "alpha of this case is not determined to the bar"
    yard = zhouse_step_longdouble(rig.column, rig.state.beta, w, k, dtype=C128)
    wimage, bimage = _prepare(rig, k, w, wcol)
    c0 = _counts(hip)
    out = hip.zhouse_step(rig.Hv, rig.Beta, rig.V, rig.W, wcol, k, slot)
    c1 = _counts(hip)
    assert out is not None and out is not False, "step k = %d at n = %d: %r" % (k, n, out)
    assert out.shape == (k + 6,) and out.dtype == C128
    u, v = rig.Hv.download(k + 1, 1)[:, 0], rig.V.download(k + 1, 1)[:, 0]
    try:
        errs, bars = assert_zstep_matches(_as_zstep(out, u, v, k), ref, yard, k, wnorm)
    except AssertionError as e:
        raise AssertionError("n = %d, wcol = %d, slot = %d: %s" % (n, wcol, slot, e))
    print("n = %d, k = %d, |gamma|/||w|| = %.1e: " % (n, k, abs(complex(ref.gamma)) / wnorm)
          + ", ".join("%s %.1e/%.1e" % (q, errs[q], bars[q]) for q in QS))
    _record(n, k, errs, bars)
    assert rig.Beta.get(0, k + 1, 1)[0] == float(ref.beta), "beta[k+1] on the device"
    if structure:
        _check_untouched(rig, k, wimage, bimage, targets_too=False)
    assert c1[1] == c0[1], "the launch reported a timed-out sum"
    assert c1[2] == c0[2], "n_house_chain counts the real kernel only"
    expect_kernel(c1[0] - c0[0] == 1, "k_zhouse_chain launches for n = %d, k = %d: %d" % (n, k, c1[0] - c0[0]))
    _restore(rig, k)
    return out, u, v, ref


def _skip_if_not_served():
    if not SERVED:
        pytest.skip(NOT_SERVED)


# ---- depth: 4 rows per lane, to the last served step ----
@pytest.mark.parametrize("n,ks", [(4099, [0, 1, 7, 62, 63, 511, 512, LIMIT_K - 1, LIMIT_K]),     # padded, three workgroups
                                  (70001, [0, 1, 7, 62, 63, LIMIT_K - 1, LIMIT_K]),             # padded, 35 workgroups
                                  (2001, [0, 1, 7, 62, 63, LIMIT_K - 1, LIMIT_K]),              # MASKED, one workgroup
                                  (1025, [0, 1, 7, 62, 63, LIMIT_K - 1, LIMIT_K])])                # MASKED; k = 1022 leaves one row behind k + 1
def test_depth(hip, n, ks):
    rig = _Rig(hip, n, LIMIT_K + 2, seed=n)
    for k in sorted(ks, reverse=True):          # (downwards: step k overwrites column k + 1, which no smaller k reads)
        w, ref = _pick_w(rig, k, seed=n)
        _step(rig, k, w, ref)
    # k + 2 > 1024: declined, whatever else is switched on
    _declined(rig, LIMIT_K + 1, _crandn(np.random.default_rng(n), n))
    _skip_if_not_served()


# ---- every rows-per-lane class ----
def _class_sizes(hip):
    """The smallest odd complex length of every rows-per-lane class of ``chain_geometry`` on this device (a class holds
    ``rows * 512 * CUs`` complex rows), and whether ``k_zhouse_chain`` serves it (house.hip: up to 32 rows)."""
    ncu = hip.info()["compute_units"]
    out, prev = [], 0
    for rows in (4, 8, 16, 24, 32, 40):
        out.append((rows, prev * 512 * ncu + 4099, rows <= 32))
        prev = rows
    return out


@pytest.mark.parametrize("cls", range(6))
def test_every_rows_per_lane_class(hip, cls):
    rows, n, served = _class_sizes(hip)[cls]
    t0 = time.time()
    rig = _Rig(hip, n, 9, seed=n)
    w, ref = _pick_w(rig, 8, seed=n)
    if served:
        _step(rig, 8, w, ref)
    else:
        _declined(rig, 8, w)          # 40 rows per lane: the instantiation spills in its streaming loops and is not shipped
    print("%d rows per lane, n = %d: %.1f s of host time" % (rows, n, time.time() - t0))
    _skip_if_not_served()


# ---- zero factors: links that are skipped ----
_ZERO = {"first": [0], "last": [8], "run": [3, 4, 5], "ends": [0, 1, 7, 8], "all_but_one": [0, 1, 2, 3, 5, 6, 7, 8],
         "all": list(range(9))}


@pytest.mark.parametrize("pattern", sorted(_ZERO))
def test_zero_factors(hip, pattern):
    n = 70001
    rig = _Rig(hip, n, 9, seed=n + 1, zero_beta=_ZERO[pattern])
    w, ref = _pick_w(rig, 8, seed=n + 1)
    _step(rig, 8, w, ref)
    _skip_if_not_served()


def _no_link_rig(hip, n, seed):
    return _Rig(hip, n, 9, seed=seed, zero_beta=range(9))


@pytest.mark.parametrize("n", [2001, 70001])
def test_no_link_at_all_gamma_zero(hip, n):
    """Every factor zero and w[k+1] == 0 exactly: the branch gamma == 0, sigma != 0 (v0 = -sigma, alpha = 1)."""
    rig = _no_link_rig(hip, n, n + 2)
    w = _crandn(np.random.default_rng(n + 2), n)
    w[9] = 0.0
    got = _step(rig, 8, w)
    _skip_if_not_served()
    out, u, v, ref = got
    assert ref.gamma == 0 and ref.beta == 2 and ref.alpha == 1
    assert out[9] == 0 and out[12] == 1 and u[9].real < 0 and u[9].imag == 0
    bits_equal(out[:9], w[:9], "raw rows without any link")


@pytest.mark.parametrize("gamma", [1.5, -0.75, 1.25j, -2.0j])
def test_no_link_at_all_purely_real_or_imaginary_gamma(hip, gamma):
    """gamma on an axis: |gamma| is exact, alpha = -gamma / |gamma| is -1, +1, -i, +i exactly."""
    n = 70001
    rig = _no_link_rig(hip, n, n + 5)
    w = _crandn(np.random.default_rng(n + 5), n)
    w[9] = gamma
    got = _step(rig, 8, w)
    _skip_if_not_served()
    out, u, v, ref = got
    assert out[9] == gamma and out[12] == -gamma / abs(gamma) and out[13] == 2


@pytest.mark.parametrize("n", [2001, 70001])
def test_no_link_at_all_exact_breakdown_at_k5(hip, n):
    """Every factor zero and w[k+1:] == 0: everything finite, the new reflector is e_{k+1}, beta = 0."""
    k = 5
    rig = _no_link_rig(hip, n, n + 3)
    w = _crandn(np.random.default_rng(n + 3), n)
    w[k + 1:] = 0.0
    got = _step(rig, k, w)
    _skip_if_not_served()
    out, u, v, ref = got
    e = np.zeros(n, dtype=C128)
    e[k + 1] = 1.0
    assert np.array_equal(u, e) and np.array_equal(v, e)
    assert np.array_equal(out, np.concatenate([w[: k + 1], [0.0, 0.0, 0.0, 1.0, 0.0]]))


# ---- tiny vectors ----
@pytest.mark.parametrize("n", [2, 3, 64, 65])
def test_tiny_vectors(hip, n):
    rig = _Rig(hip, n, n - 1, seed=n + 4)
    for k in sorted({0, (n - 2) // 2, n - 2}, reverse=True):
        w, ref = _pick_w(rig, k, seed=n + 4)
        if k == n - 2:       # the last served step: nothing behind row k + 1
            assert ref.sigma2 == 0 and ref.beta == 0
        got = _step(rig, k, w, ref)
        if got is not None and k == n - 2:
            assert got[0][k + 2] == 0 and got[0][k + 5] == 0 and got[1][n - 1] == 1
    _declined(rig, n - 1, _crandn(np.random.default_rng(n), n))          # k + 1 >= n
    _skip_if_not_served()


# ---- plumbing ----
def test_w_column_1_of_3(hip):
    rig = _Rig(hip, 4099, 9, seed=21, wcols=3)
    rng = np.random.default_rng(22)
    rig.W.upload(0, rng.standard_normal((4099, 3)) + 1j * rng.standard_normal((4099, 3)))
    w, ref = _pick_w(rig, 8, seed=21)
    _step(rig, 8, w, ref, wcol=1)          # (the W image compared afterwards has all three columns)
    _skip_if_not_served()


@pytest.mark.parametrize("slot", [1, 2, 3])
def test_slots(hip, slot):
    rig = _Rig(hip, 4099, 9, seed=23)
    w, ref = _pick_w(rig, 8, seed=23)
    _step(rig, 8, w, ref, slot=slot)
    _skip_if_not_served()


def test_the_same_call_twice_gives_the_same_bits(hip):
    rig = _Rig(hip, 70001, 66, seed=26)
    w, ref = _pick_w(rig, 64, seed=26)
    first = _step(rig, 64, w, ref)
    second = _step(rig, 64, w, ref, structure=False)
    _skip_if_not_served()
    for a, b, what in zip(first[:3], second[:3], ("returned column", "reflector", "basis column")):
        bits_equal(b, a, what)


def test_real_blocks_are_not_taken(hip):
    """``zhouse_step`` checks the dtypes itself: a real basis is for ``house_step``."""
    Hv, V, W, Beta = hip.alloc(64, 4), hip.alloc(64, 4), hip.alloc(64, 1), hip.alloc(4, 1)
    c0 = _counts(hip)
    assert hip.zhouse_step(Hv, Beta, V, W, 0, 0) is None and _counts(hip) == c0


# ---- a timed-out sum ----
def test_timed_out_launch_is_recovered_on_the_per_reflector_path(hip):
    """``chain_fault`` sets the error word the kernel reads (nothing hangs): the direct call returns False, and an Arnoldi
    run that meets it at step 5 re-runs that step per reflector - held to the same step-local bars as a served step - and
    agrees with the run that never used the kernel."""
    n = 70001
    rig = _Rig(hip, n, 9, seed=28)
    w, ref = _pick_w(rig, 8, seed=28)
    try:
        if SERVED:
            _prepare(rig, 8, w, 0)
            c0 = _counts(hip)
            hip.set("chain_fault", 1)
            assert hip.zhouse_step(rig.Hv, rig.Beta, rig.V, rig.W, 0, 8) is False
            c1 = _counts(hip)
            assert c1[0] - c0[0] == 1 and c1[1] - c0[1] == 1 and c1[2] == c0[2]
            bits_equal(rig.W.download(), w.reshape(-1, 1), "W after a timed-out launch")
            _restore(rig, 8)
            _step(rig, 8, w, ref)          # the next launch is served again and meets the bars
        import scipy.sparse as sp
        A = sp.diags([-1.3 + 0.2j, 2.0 + 1.0j, -0.7, 0.25j], [-1, 0, 1, 7], shape=(n, n)).tocsr()
        v = _crandn(np.random.default_rng(29), n).reshape(-1, 1)

        caught = {}

        def run(fault_at=None):
            """8 steps; at ``fault_at`` the launch is faked to time out, the state it was given is kept, and the step the
            host then re-runs per reflector is held to the step-local bars."""
            ar = utils.Arnoldi(A, v, maxiter=8, ortho="house")
            inner = hip.zhouse_step

            def spy(Hv, Beta, V, W, wcol, k, slot=0):
                if k != fault_at or not SERVED:
                    return inner(Hv, Beta, V, W, wcol, k, slot)
                caught.update(U=Hv.download(0, k + 1), beta=Beta.download()[: k + 1, 0], w=W.download(wcol, 1)[:, 0])
                hip.set("chain_fault", 1)
                out = inner(Hv, Beta, V, W, wcol, k, slot)
                assert out is False, "the faked timeout was not reported: %r" % (out,)
                return out

            hip.zhouse_step = spy
            try:
                while ar.iter < 8:
                    ar.advance()
            finally:
                del hip.zhouse_step
            if caught:
                k, U = fault_at, caught["U"]
                cols = lambda j: U[:, j]            # noqa: E731
                sref = zhouse_step_longdouble(cols, caught["beta"], caught["w"], k)
                yard = zhouse_step_longdouble(cols, caught["beta"], caught["w"], k, dtype=C128)
                h = ar.houses[k + 1]
                assert type(h) is utils._DevHouse, "step %d was not re-run per reflector" % k
                # H[:k+1, k] = raw * conj(alpha_j) with |alpha_j| = 1: raw = H * alpha_j (one more rounding per entry);
                # gamma and sigma^2 are not kept by the per-reflector path
                alphas = np.array([complex(x.alpha) for x in ar.houses[: k + 1]])
                got = ZStep(np.asarray(ar.H)[: k + 1, k] * alphas, None, None, h.xnorm, h.alpha, h.beta,
                            ar._Hv.download(k + 1, 1)[:, 0], ar._V.download(k + 1, 1)[:, 0])
                errs, bars = assert_zstep_matches(got, sref, yard, k, float(np.linalg.norm(caught["w"])))
                print("re-run of the timed-out step %d per reflector: " % k
                      + ", ".join("%s %.1e/%.1e" % (q, errs[q], bars[q]) for q in QS if q in errs))
            return ar

        hip.set("house_chain", 0)
        old = run()
        hip.set("house_chain", 1)
        c0 = _counts(hip)
        new = run(fault_at=5)
        c1 = _counts(hip)
    finally:
        hip.set("chain_fault", 0)
        hip.set("house_chain", 1)        # (starts the context's count of timeouts again)
    print("recovered run against the per-reflector run: rel(H) = %.2e, rel(V) = %.2e" % (crel(new.H, old.H), crel(new.V, old.V)))
    assert np.all(np.isfinite(new.H)) and np.all(np.isfinite(new.V))
    assert crel(new.H, old.H) < RTOL and crel(new.V, old.V) < RTOL
    if SERVED:
        assert c1[1] - c0[1] == 1 and c1[0] - c0[0] == 8 and c1[2] == c0[2]      # (the faulted launch counts as one)
