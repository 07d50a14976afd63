"""GPU tests of ``k_house_chain`` (krypy_amd/csrc/house.h) against an extended-precision reference written outside the
package (``tests/support/house_ref.py``), to the last served step ``k = 1022``.

``hip.house_step`` is called DIRECTLY on constructed state - seeded unit reflector columns, factors 2.0 or 0.0, a random
``w`` - so that every boundary of the kernel is reached without running a thousand Arnoldi steps first: wave boundaries
(``k + 1`` = 127, 128), the last lane (``k + 1`` = 1022, 1023), the decline at ``k + 2 > 1024``, every rows-per-lane class, runs
of skipped links, the scalar branches, tiny vectors, the plumbing (``wcol``, slots, ``tag_wait``, an epoch wrap).  Then the
public path (``Arnoldi`` / ``Gmres`` with ``ortho='house'``) at that depth.

THE BAR (``house_ref.assert_step_matches``), for every compared quantity: ``16 x max(E64, eps sqrt(k + 2))``, ``eps = 2.2e-16``.
``E64`` is the error of a float64 NumPy evaluation of the same step on the same inputs against the extended-precision one,
computed in the test; the factor 16 covers another order of summation (serial FMAs per lane, then DPP and LDS trees, against
NumPy's pairwise sums).  Neither figure comes from the device.  ``raw[0..k]`` and ``gamma``: max-abs error over ``||w||``;
``sigma^2`` and ``xnorm``: relative; ``alpha`` and ``beta_{k+1}``: exact; ``u_{k+1}`` and ``v_{k+1}``: 2-norm of the difference.
Every case with ``gamma != 0`` has ``|gamma_ref| >= 1e-6 ||w||`` (asserted; reseeded otherwise), so the sign branch cannot
flip from rounding.  The device's own errors are printed per case and as a table at the end of the module
(``HOUSE-STEP DEVICE ERRORS``; KERNELS.md 4.20 quotes one run).

With ``KRYPY_AMD_TEST_FORCE_MULTI=1`` the kernel declines: a direct call must return ``None`` and leave every block bit for
bit as it was - that is checked, then the numeric part of the direct-call tests is skipped (a direct call has no
per-reflector form); the ``Arnoldi`` / ``Gmres`` tests run on the per-reflector path."""
import time

import numpy as np
import pytest

from krypy_amd import linsys, utils
from tests.parity_cases import RTOL, check_resnorms, rel
from tests.support.house_ref import (Step, assert_step_matches, house_arnoldi_longdouble, house_step_longdouble,
                                     reflector_state)
from tests.support.kernel_expect import expect_kernel
from tests.support.poison import bits_equal, poisoned_allocations
from tests.test_gpu_house import (SERVED, _banded, _check_reference_inequalities, _convection_diffusion, _counts,
                                  _per_reflector, _run)

pytestmark = pytest.mark.gpu

JUNK = -3.25                 # what the two target columns and beta[k+1] hold before a call
DEPTH_KS = [0, 1, 2, 3, 62, 63, 64, 125, 126, 127, 128, 129, 510, 511, 512, 1020, 1021, 1022]
NOT_SERVED = "KRYPY_AMD_TEST_FORCE_MULTI=1: house_step declines (checked: None, blocks untouched); a direct call has no " \
             "per-reflector form to run the numeric part on"

_measured = {}               # (quantity, n) -> (largest device error, its bar, k)


@pytest.fixture(scope="module", autouse=True)
def _report_device_errors():
    t0 = time.time()
    yield
    print("\nHOUSE-STEP DEVICE ERRORS (largest per quantity and length; bar of that case; k of that case)")
    for n in sorted({key[1] for key in _measured}):
        print("  n = %-9d" % n + "  ".join("%s %.2e / %.2e (k=%d)" % ((q,) + _measured[(q, n)])
                                           for q in ("raw", "gamma", "sigma2", "xnorm", "u", "v") if (q, n) in _measured))
    print("HOUSE-STEP MODULE WALL TIME %.1f s" % (time.time() - t0))


def _record(n, k, errs, bars):
    for q, e in errs.items():
        if (q, n) not in _measured or e > _measured[(q, n)][0]:
            _measured[(q, n)] = (e, bars[q], k)


class _Rig(object):
    """Device blocks for direct calls on a constructed state of ``ncols`` reflectors of length ``n``: ``Hv`` and ``V`` have
    ``ncols + 3`` columns (step ``k = ncols - 1`` writes column ``ncols``, the sentinel sits behind it; a declined step
    ``k = ncols`` is prepared the same way), ``Beta`` ``ncols + 3`` entries.  Column ``c`` of ``V`` holds ``(c + 1) * vfill``.  A
    host copy of the reflector block is kept up to 1 GB; beyond that columns are made again from their seeds."""

    def __init__(self, hip, n, ncols, seed, zero_beta=(), wcols=1, alloc_zero=True, host_block=True):
        self.hip, self.n, self.ncols = hip, n, ncols
        self.state = reflector_state(n, ncols, seed, zero_beta)
        upto = ncols
        self.Hv = hip.alloc(n, ncols + 3, zero=alloc_zero)
        self.V = hip.alloc(n, ncols + 3, zero=alloc_zero)
        self.Beta = hip.alloc(ncols + 3, 1, zero=alloc_zero)
        self.W = hip.alloc(n, wcols, zero=alloc_zero)
        self.U = self.state.block(0, upto) if host_block and 8.0 * n * upto <= 1e9 else None
        rng = np.random.default_rng([seed, 77])
        self.vfill = rng.standard_normal(n)
        self.sentinel = rng.standard_normal(n)
        for j0 in range(0, upto, 64):
            j1 = min(upto, j0 + 64)
            self.Hv.upload(j0, self.U[:, j0:j1] if self.U is not None else self.state.block(j0, j1))
        if alloc_zero:
            for c0 in range(0, ncols + 3, 64):
                cs = np.arange(c0, min(ncols + 3, c0 + 64))
                self.V.upload(c0, self.vfill[:, None] * (cs + 1.0)[None, :])
        self.small = float(n) * (ncols + 3) <= 2e7

    def column(self, j):
        return self.U[:, j] if self.U is not None else self.state.column(j)

    def beta_image(self, k):
        b = np.full(self.ncols + 3, 0.125)
        b[: self.ncols] = self.state.beta
        b[k + 1] = JUNK
        return b


def _pick_w(rig, k, seed):
    """A random ``w`` whose reference ``gamma`` is well away from zero (reseeded otherwise), and its reference step."""
    for attempt in range(6):
        w = np.random.default_rng([seed, k, attempt]).standard_normal(rig.n)
        ref = house_step_longdouble(rig.column, rig.state.beta, w, k)
        if abs(float(ref.gamma)) >= 1e-6 * float(np.linalg.norm(w)):
            return w, ref
    raise AssertionError("no w with |gamma| >= 1e-6 ||w|| in six seeds: n = %d, k = %d" % (rig.n, k))


def _v_column(rig, c):
    return rig.vfill * (c + 1.0)


def _check_untouched(rig, k, wimage, bimage, targets_too):
    """Columns 0 .. k and the sentinel column of Hv, every column of V but k + 1 (a sample of three when the block is large),
    W, Beta but entry k + 1, the padding of all of them; ``targets_too``: the call was declined - the target columns and
    beta[k+1] still hold what they held."""
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
        junk = np.full(rig.n, JUNK)
        bits_equal(rig.Hv.download(k + 1, 1)[:, 0], junk, "reflector column k + 1 of a declined step")
        bits_equal(rig.V.download(k + 1, 1)[:, 0], junk, "basis column k + 1 of a declined step")
        assert b[k + 1] == JUNK
    assert rig.Hv.padding_nonzero() == 0 and rig.V.padding_nonzero() == 0 and rig.Beta.padding_nonzero() == 0


def _prepare(rig, k, w, wcol):
    junk = np.full(rig.n, JUNK)
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
    out = rig.hip.house_step(rig.Hv, rig.Beta, rig.V, rig.W, wcol, k, slot)
    assert out is None, "step k = %d at n = %d was not declined" % (k, rig.n)
    assert _counts(rig.hip) == c0
    _check_untouched(rig, k, wimage, bimage, targets_too=True)
    _restore(rig, k)


def _step(rig, k, w, ref=None, wcol=0, slot=0, signs=None, structure=True):
    """One served call, compared with the reference and checked for what it must not touch.  Returns
    ``(out, u, v, ref)`` - or None when the kernel is switched off for the whole run (FORCE_MULTI)."""
    hip, n = rig.hip, rig.n
    if not SERVED:
        _declined(rig, k, w, wcol, slot)
        return None
    if ref is None:
        ref = house_step_longdouble(rig.column, rig.state.beta, w, k)
    wnorm = float(np.linalg.norm(w))
    assert ref.gamma == 0 or abs(float(ref.gamma)) >= 1e-6 * wnorm, "the sign branch of this case could flip from rounding"
    if signs is not None:
        signs.add(float(np.sign(ref.gamma)))
    yard = house_step_longdouble(rig.column, rig.state.beta, w, k, dtype=np.float64)
    wimage, bimage = _prepare(rig, k, w, wcol)
    c0 = _counts(hip)
    out = hip.house_step(rig.Hv, rig.Beta, rig.V, rig.W, wcol, k, slot)
    c1 = _counts(hip)
    assert out is not None and out is not False, "step k = %d at n = %d: %r" % (k, n, out)
    assert out.shape == (k + 6,)
    u, v = rig.Hv.download(k + 1, 1)[:, 0], rig.V.download(k + 1, 1)[:, 0]
    got = Step(out[: k + 1], out[k + 1], out[k + 2], out[k + 3], out[k + 4], out[k + 5], u, v)
    try:
        errs, bars = assert_step_matches(got, ref, yard, k, wnorm)
    except AssertionError as e:
        raise AssertionError("n = %d, wcol = %d, slot = %d: %s" % (n, wcol, slot, e))
    print("n = %d, k = %d, gamma/||w|| = %+.1e: " % (n, k, float(ref.gamma) / wnorm)
          + ", ".join("%s %.1e/%.1e" % (q, errs[q], bars[q]) for q in ("raw", "gamma", "sigma2", "xnorm", "u", "v")))
    _record(n, k, errs, bars)
    assert rig.Beta.get(0, k + 1, 1)[0] == float(ref.beta), "beta[k+1] on the device"
    if structure:
        _check_untouched(rig, k, wimage, bimage, targets_too=False)
    assert c1[1] == c0[1], "the launch reported a timed-out sum"
    expect_kernel(c1[0] - c0[0] == 1, "k_house_chain launches for n = %d, k = %d: %d" % (n, k, c1[0] - c0[0]))
    _restore(rig, k)
    return out, u, v, ref


def _skip_if_not_served():
    if not SERVED:
        pytest.skip(NOT_SERVED)


# ---- depth: 4 rows per lane, to the last served step ----
@pytest.mark.parametrize("n,ks", [(4099, DEPTH_KS),        # padded, the second workgroup almost all padding
                                  (70001, DEPTH_KS),
                                  (3001, [0, 1, 127, 128, 1021, 1022]),       # MASKED
                                  (1025, [0, 1, 127, 128, 1021, 1022])])      # MASKED; k = 1022 leaves one row behind k + 1
def test_depth(hip, n, ks):
    rig = _Rig(hip, n, 1024, seed=n)
    signs = set()
    for k in sorted(ks, reverse=True):          # (downwards: step k overwrites column k + 1, which no smaller k reads)
        w, ref = _pick_w(rig, k, seed=n)
        _step(rig, k, w, ref, signs=signs)
    # k + 2 > 1024: declined, whatever else is switched on
    _declined(rig, 1023, np.random.default_rng(n).standard_normal(n))
    _skip_if_not_served()
    assert signs == {-1.0, 1.0}, "both signs of gamma must occur over the case list: %r" % signs


# ---- every rows-per-lane class ----
@pytest.mark.parametrize("n", [3001, 1000003, 1100001, 2200000, 4300000, 6400000, 10000000])
def test_every_rows_per_lane_class(hip, n):
    t0 = time.time()
    rig = _Rig(hip, n, 9, seed=n, host_block=n < 1000000)          # (the long columns are made again from their seeds)
    w, ref = _pick_w(rig, 8, seed=n)
    _step(rig, 8, w, ref)
    print("n = %d: %.1f s of host time" % (n, time.time() - t0))
    _skip_if_not_served()


def test_eight_rows_per_lane_across_a_wave_boundary(hip):
    n = 1100001
    rig = _Rig(hip, n, 129, seed=8)
    for k in (128, 127):
        w, ref = _pick_w(rig, k, seed=8)
        _step(rig, k, w, ref)
    _skip_if_not_served()


# ---- zero factors: links that are skipped ----
_ZERO = {"first": [0], "last": [8], "run": [3, 4, 5], "ends": [0, 1, 7, 8], "all_but_one": [0, 1, 2, 3, 5, 6, 7, 8],
         "all": list(range(9))}


@pytest.mark.parametrize("n", [70001, 2200000])
@pytest.mark.parametrize("pattern", sorted(_ZERO))
def test_zero_factors(hip, n, pattern):
    rig = _Rig(hip, n, 9, seed=n + 1, zero_beta=_ZERO[pattern])
    w, ref = _pick_w(rig, 8, seed=n + 1)
    _step(rig, 8, w, ref)
    _skip_if_not_served()


@pytest.mark.parametrize("n", [70001, 2200000])
def test_no_link_at_all_gamma_zero(hip, n):
    """Every factor zero and w[k+1] == 0.0 exactly: the branch gamma == 0, sigma != 0 (v0 = -sigma, alpha = 1)."""
    rig = _Rig(hip, n, 9, seed=n + 2, zero_beta=range(9))
    w = np.random.default_rng(n + 2).standard_normal(n)
    w[9] = 0.0
    got = _step(rig, 8, w)
    _skip_if_not_served()
    out, u, v, ref = got
    assert ref.gamma == 0 and ref.beta == 2 and ref.alpha == 1
    assert out[9] == 0.0 and out[12] == 1.0 and u[9] < 0
    bits_equal(out[:9], w[:9], "raw rows without any link")


@pytest.mark.parametrize("n", [70001, 2200000])
def test_no_link_at_all_exact_breakdown_at_k5(hip, n):
    """Every factor zero and w[k+1:] == 0: everything finite, the new reflector is e_{k+1}, beta = 0."""
    k = 5
    rig = _Rig(hip, n, 9, seed=n + 3, zero_beta=range(9))
    w = np.random.default_rng(n + 3).standard_normal(n)
    w[k + 1:] = 0.0
    got = _step(rig, k, w)
    _skip_if_not_served()
    out, u, v, ref = got
    e = np.zeros(n)
    e[k + 1] = 1.0
    bits_equal(u, e, "the new reflector")
    bits_equal(v, e, "the new basis column")
    bits_equal(out, np.concatenate([w[: k + 1], [0.0, 0.0, 0.0, 1.0, 0.0]]), "the returned column")


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
            assert got[0][k + 2] == 0.0 and got[0][k + 5] == 0.0 and abs(got[1][n - 1]) == 1.0
    _declined(rig, n - 1, np.random.default_rng(n).standard_normal(n))          # k + 1 >= n
    _skip_if_not_served()


# ---- plumbing ----
def test_w_column_1_of_3(hip):
    rig = _Rig(hip, 4099, 9, seed=21, wcols=3)
    rig.W.upload(0, np.random.default_rng(22).standard_normal((4099, 3)))
    w, ref = _pick_w(rig, 8, seed=21)
    _step(rig, 8, w, ref, wcol=1)          # (the W image compared afterwards has all three columns)
    _skip_if_not_served()


@pytest.mark.parametrize("slot", [1, 2, 3])
def test_slots(hip, slot):
    rig = _Rig(hip, 4099, 9, seed=23)
    w, ref = _pick_w(rig, 8, seed=23)
    _step(rig, 8, w, ref, slot=slot)
    _skip_if_not_served()


def test_without_the_completion_tag(hip):
    rig = _Rig(hip, 4099, 9, seed=24)
    tag = hip.get("tag_wait")
    hip.set("tag_wait", 0)
    try:
        for k, slot in ((8, 0), (7, 2)):
            w, ref = _pick_w(rig, k, seed=24)
            _step(rig, k, w, ref, slot=slot)
    finally:
        hip.set("tag_wait", tag)
    w, ref = _pick_w(rig, 6, seed=24)
    _step(rig, 6, w, ref)          # (and with the tag again)
    _skip_if_not_served()


def test_epoch_wrap_in_front_of_a_deep_step(hip):
    """The epoch counter 5 short of the wrap threshold: the first launch carries it past (by 2 k + 3 = 2003), the check in
    front of the second one zeroes the granules and starts over."""
    rig = _Rig(hip, 4099, 1001, seed=25)
    w, ref = _pick_w(rig, 1000, seed=25)
    wraps = hip.get("n_epoch_wraps")
    if SERVED:
        hip.set("chain_epoch", 0xfff00000 - 5)
    first = _step(rig, 1000, w, ref)
    second = _step(rig, 1000, w, ref)
    _skip_if_not_served()
    assert hip.get("n_epoch_wraps") == wraps + 1
    for a, b, what in zip(first[:3], second[:3], ("returned column", "reflector", "basis column")):
        bits_equal(b, a, what + " after the wrap")


def test_the_same_call_twice_gives_the_same_bits(hip):
    rig = _Rig(hip, 70001, 130, seed=26)
    w, ref = _pick_w(rig, 128, seed=26)
    first = _step(rig, 128, w, ref)
    second = _step(rig, 128, w, ref, structure=False)
    _skip_if_not_served()
    for a, b, what in zip(first[:3], second[:3], ("returned column", "reflector", "basis column")):
        bits_equal(b, a, what)


@pytest.mark.parametrize("k", [128, 1022])
def test_poisoned_targets(hip, k):
    """Blocks handed out unzeroed and full of NaN, only columns 0 .. k, the factors and w uploaded: the bits of the run on
    clean blocks - nothing unwritten is read - and the padding stays zero."""
    n = 70001
    clean = _Rig(hip, n, k + 1, seed=27)
    w, ref = _pick_w(clean, k, seed=27)
    got = _step(clean, k, w, ref, structure=False)
    _skip_if_not_served()
    c0 = _counts(hip)
    with poisoned_allocations(hip) as rec:
        dirty = _Rig(hip, n, k + 1, seed=27, alloc_zero=False)
        assert rec.poisoned == 4
        b = np.full(k + 4, np.nan)
        b[: k + 1] = dirty.state.beta
        dirty.Beta.upload(0, b)
        dirty.W.upload(0, w)
        out = hip.house_step(dirty.Hv, dirty.Beta, dirty.V, dirty.W, 0, k, 0)
        bits_equal(out, got[0], "returned column")
        bits_equal(dirty.Hv.download(k + 1, 1)[:, 0], got[1], "reflector")
        bits_equal(dirty.V.download(k + 1, 1)[:, 0], got[2], "basis column")
        nan = np.full(n, np.nan)
        bits_equal(dirty.Hv.download(k + 2, 1)[:, 0], nan, "the column behind the new reflector")
        bits_equal(dirty.V.download(k, 1)[:, 0], nan, "basis column k")
        bits_equal(dirty.V.download(k + 2, 1)[:, 0], nan, "basis column k + 2")
        bits_equal(dirty.Hv.download(0, k + 1), dirty.U, "reflector columns")
        assert dirty.Beta.get(0, k + 1, 1)[0] == float(ref.beta)
        assert dirty.Hv.padding_nonzero() == 0 and dirty.V.padding_nonzero() == 0 and dirty.Beta.padding_nonzero() == 0
    c1 = _counts(hip)
    assert c1[1] == c0[1]
    expect_kernel(c1[0] - c0[0] == 1, "k_house_chain launches on poisoned blocks: %d" % (c1[0] - c0[0]))


# ---- the public path at depth ----
def _spy_on_steps(hip, checked, seen):
    """Wrap ``hip.house_step``: the steps in ``checked`` are compared with the reference fed the state downloaded before the
    step.  Returns the function that takes the wrapper off again."""
    inner = hip.house_step

    def spy(Hv, Beta, V, W, wcol, k, slot=0):
        if k not in checked or not SERVED:
            return inner(Hv, Beta, V, W, wcol, k, slot)
        U = Hv.download(0, k + 1)
        beta = Beta.download()[: k + 1, 0]
        w = W.download(wcol, 1)[:, 0]
        out = inner(Hv, Beta, V, W, wcol, k, slot)
        assert out is not None and out is not False, "step %d: %r" % (k, out)
        cols = lambda j: U[:, j]            # noqa: E731
        ref = house_step_longdouble(cols, beta, w, k)
        yard = house_step_longdouble(cols, beta, w, k, dtype=np.float64)
        wnorm = float(np.linalg.norm(w))
        assert ref.gamma == 0 or abs(float(ref.gamma)) >= 1e-6 * wnorm
        got = Step(out[: k + 1], out[k + 1], out[k + 2], out[k + 3], out[k + 4], out[k + 5], Hv.download(k + 1, 1)[:, 0],
                   V.download(k + 1, 1)[:, 0])
        errs, bars = assert_step_matches(got, ref, yard, k, wnorm)
        print("Arnoldi n = %d, step %d: " % (V.n, k)
              + ", ".join("%s %.1e/%.1e" % (q, errs[q], bars[q]) for q in ("raw", "gamma", "sigma2", "xnorm", "u", "v")))
        _record(V.n, k, errs, bars)
        assert Beta.get(0, k + 1, 1)[0] == float(ref.beta)
        seen.append(k)
        return out

    hip.house_step = spy

    def undo():
        del hip.house_step

    return undo


@pytest.mark.parametrize("n", [4099, 70001])
def test_arnoldi_1030_steps(hip, n):
    steps = 1030
    A = _banded(n)
    v = np.random.default_rng(n + 30).standard_normal(n)
    checked = sorted(set(range(0, 1023, 64)) | set(DEPTH_KS))
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
    orth = _check_reference_inequalities(A, V, H)
    assert np.count_nonzero(np.tril(H, -2)) == 0 and np.all(np.diag(H, -1) >= 0)
    with _per_reflector(hip):
        old = _run(A, v, 200)
    Vo, Ho = old.get()
    o_new = np.linalg.norm(np.eye(201) - V[:, :201].T.dot(V[:, :201]), 2)
    o_old = np.linalg.norm(np.eye(201) - Vo.T.dot(Vo), 2)
    print("n = %d: ||I - V^T V||_2 = %.3e over 1031 columns, %.3e over the first 201 (per-reflector run: %.3e)" % (
        n, orth, o_new, o_old))
    assert o_new <= 4 * o_old, (o_new, o_old)
    # the first 40 steps against the extended-precision run (further on the basis is not determined to rounding)
    Hl, Vl, _, _, _ = house_arnoldi_longdouble(A, v, 40)
    assert rel(H[:41, :40], Hl) < RTOL and rel(V[:, :41], Vl) < RTOL
    assert c1[1] == c0[1], "a launch reported a timed-out sum"
    # steps 0 .. 1022 are served, 1023 .. 1029 fall to the per-reflector path on the same object
    expect_kernel(c1[0] - c0[0] == (1023 if SERVED else 0), "k_house_chain launches in 1030 steps: %d" % (c1[0] - c0[0]))


_alternating = {}


def _alternating_runs(hip):
    """40 steps of a Householder and of a modified Gram-Schmidt Arnoldi object (n = 250,000; the latter with its look-ahead
    step in flight), each alone and then advanced alternately on the one context: they share the granules, the epoch counter
    and the step slots.  Run once, shared by the two tests below."""
    if not _alternating:
        steps = 40
        A = _convection_diffusion(500)
        v = np.random.default_rng(31).standard_normal((A.shape[0], 1))
        alone_h = utils.Arnoldi(A, v, maxiter=steps, ortho="house")
        for _ in range(steps):
            alone_h.advance()
        alone_m = utils.Arnoldi(A, v, maxiter=steps, ortho="mgs")
        for _ in range(steps):
            alone_m.advance()
        c0, r0 = _counts(hip), hip.get("n_blk_rebuild")
        both_h = utils.Arnoldi(A, v, maxiter=steps, ortho="house")
        both_m = utils.Arnoldi(A, v, maxiter=steps, ortho="mgs")
        for _ in range(steps):
            both_h.advance()
            both_m.advance()
        c1 = _counts(hip)
        pick = lambda ar: (np.array(ar.H), np.array(ar.V))            # noqa: E731
        _alternating.update(house=(pick(both_h), pick(alone_h)), mgs=(pick(both_m), pick(alone_m)), steps=steps,
                            launches=c1[0] - c0[0], recovered=c1[1] - c0[1], rebuilds=hip.get("n_blk_rebuild") - r0)
    return _alternating


def test_house_history_is_unchanged_by_interleaved_mgs_steps(hip):
    r = _alternating_runs(hip)
    (H, V), (H0, V0) = r["house"]
    print("house, alternating against alone: rel(H) = %.3e, rel(V) = %.3e" % (rel(H, H0), rel(V, V0)))
    bits_equal(H, H0, "house H")
    bits_equal(V, V0, "house V")
    assert rel(H0, r["mgs"][1][0]) < 1e-8          # (and both orthogonalisations build the same Hessenberg matrix)
    assert r["recovered"] == 0
    expect_kernel(r["launches"] == (r["steps"] if SERVED else 0), "k_house_chain launches: %d" % r["launches"])


def test_mgs_history_is_unchanged_by_interleaved_house_steps(hip):
    """A Householder step claims step slot 0 and thereby settles the Gram-Schmidt object's look-ahead step whenever that one is
    parked there: waited for, its column cleared, begun again at the next ``advance``.  Clearing that column must not cost the
    blocked kernel its Gram table (``kh_vec_zero`` keeps the rows below the cleared column): rows rebuilt from the basis round
    differently from the rows computed in flight, and the history then differed from the run alone by rel(H) = 2.8e-15,
    rel(V) = 2.9e-15 (722 of 1640 words of H, first in column 14) - measured on an MI355X before ``kh_vec_zero`` was changed."""
    r = _alternating_runs(hip)
    (H, V), (H0, V0) = r["mgs"]
    print("mgs, alternating against alone: rel(H) = %.3e, rel(V) = %.3e, %d of %d words of H differ" % (
        rel(H, H0), rel(V, V0), int(np.count_nonzero(H.view(np.uint64) != H0.view(np.uint64))), H.size))
    bits_equal(H, H0, "mgs H")
    bits_equal(V, V0, "mgs V")
    print("Gram table rebuilds of the alternating Gram-Schmidt run: %d" % r["rebuilds"])


def test_gmres_house_250k(hip):
    """GMRES on the 250,000-row convection-diffusion operator to 1e-8.  The right-hand side is A^4 r (r random): without the
    smoothest modes the solve takes about 50 steps instead of 750, which the CPU oracle walks through in a second."""
    from oracle import krylov_ref as ref
    A = _convection_diffusion(500)
    n = A.shape[0]
    b = np.random.default_rng(32).standard_normal(n)
    for _ in range(4):
        b = A.dot(b)
    b = (b / np.linalg.norm(b)).reshape(-1, 1)
    tol = 1e-8
    c0 = _counts(hip)
    s = linsys.Gmres(linsys.LinearSystem(A, b), ortho="house", tol=tol, maxiter=200)
    c1 = _counts(hip)
    o = ref.gmres(A, b[:, 0], tol=tol, maxiter=200)
    assert 30 <= s.arnoldi.iter <= 200
    print("GMRES(house) at n = %d: %d iterations, %d Arnoldi steps" % (n, s.iter, s.arnoldi.iter))
    check_resnorms(s.resnorms, o.resnorms, tol=1e-8, explicit_tol=1e-4)
    x = np.asarray(s.xk[:, 0], dtype=np.longdouble)
    bl = b[:, 0].astype(np.longdouble)
    from tests.support.poison import _apply_by_diagonals
    r = bl - _apply_by_diagonals(A, x)
    final = float(np.sqrt((r * r).sum()) / np.sqrt((bl * bl).sum()))
    print("  final ||b - A x|| / ||b|| in extended precision: %.3e" % final)
    assert final <= tol
    assert c1[1] == c0[1]
    expect_kernel(c1[0] - c0[0] == (s.arnoldi.iter if SERVED else 0),
                  "k_house_chain launches: %d for %d Arnoldi steps" % (c1[0] - c0[0], s.arnoldi.iter))
