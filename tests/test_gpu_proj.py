"""Every device path of the deflation projector (``kh_proj``) against the extended-precision reference of
tests/support/proj_ref.py, at the edges of each path: the chunked kernels (chunk seams, the stride loop of the small
matrix-vector product, d = 1024), the complex ladder (8 / 4 / 2 / 1, conjugation, d = 512), the one-launch kernel
(every register shape, the workgroup counts 129 and 256 of a 256-CU chip, ragged d, one and three sweeps: the other
epoch parity), the panel passes with the one-launch kernel declining, the call forms nothing else runs, the projector
inside the Arnoldi step, and the argument errors.

Every numeric comparison is ``proj_ref.assert_matches`` (16 x max(float64 yardstick, eps sqrt(d + 1)); nothing tuned
against the device).  Every statement about which kernel ran is an ``expect_kernel``, judged after the numbers; with
``KRYPY_AMD_TEST_FORCE_MULTI=1`` the one-launch kernel declines by construction and the numbers must still hold.  Lengths
of the register shapes come from the context's CU count (tests/support/proj_cases.py).  Each case logs its errors, bars
and ratios (``KRYPY_AMD_PROJ_LOG=<file>`` appends them to a file: profiles/proj_ref_gpu.log)."""
import collections
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import proj_cases as pc
from tests.support import proj_ref as pr
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

SERVED = os.environ.get("KRYPY_AMD_TEST_FORCE_MULTI", "") != "1"      # (one rank for real: the one-launch kernel is served)

_cols = collections.OrderedDict()       # (which, n, cplx) -> block: built once per length, leading columns taken
_refs = collections.OrderedDict()       # reference and yardstick of the last few sets of inputs (the sequence of sweep
                                        # counts comes back to one): computed once, never changed


def _wide_blocks(n, cplx, ncols=None, need_v=True):
    """W and V at length n with as many columns as any table row of that length needs (generation dominates at the long
    lengths); the two most recent lengths are kept."""
    out = []
    for which in ((0, 1) if need_v else (0,)):
        key = (which, n, cplx)
        have = _cols.get(key)
        if have is None or have.shape[1] < (ncols or 0):
            have = pc.block(which, n, max(ncols or 0, have.shape[1] if have is not None else 0), cplx)
            _cols[key] = have
        _cols.move_to_end(key)
        out.append(have)
    lengths = []
    for k in reversed(_cols):
        if k[1] not in lengths:
            lengths.append(k[1])
    for k in [k for k in _cols if k[1] not in lengths[:2]]:
        del _cols[k]
    return out if need_v else out * 2


def _inputs(c, n):
    if n <= pc.HOST_LIMIT:
        return pc.inputs(c, n)
    return pc.inputs(c, n, blocks=lambda n_, cplx: _wide_blocks(n_, cplx, c.d, need_v=not c.w_is_v))


def _reference(c, n, inp):
    key = (n, c.d, c.cplx, c.iterations, c.T, c.WRH, c.w_is_v)
    if key not in _refs:
        ref = pr.complement(inp.W, inp.V, c.d, inp.T, inp.WRH, c.iterations, inp.a)
        yard = pr.complement(inp.W, inp.V, c.d, inp.T, inp.WRH, c.iterations, inp.a, dtype=np.float64)
        for x in ref + yard:
            x.setflags(write=False)
        _refs[key] = (ref, yard)
        while len(_refs) > 4:           # (extended-precision vectors of up to 14.7 M entries: not kept for the session)
            _refs.popitem(last=False)
    _refs.move_to_end(key)
    return _refs[key]


def _counters(hip):
    return hip.get("n_proj_reg"), hip.get("n_proj_panel")


def _log(name, n, d, moved, hip, errs, bars):
    line = "%-36s n=%-9d d=%-5d n_proj_reg+%d n_proj_panel+%d why=%d rows=%d |" % (
        name, n, d, moved[0], moved[1], hip.get("proj_reg_why"), hip.get("proj_reg_rows"))
    for q in sorted(errs):
        line += " %s err %.3e bar %.3e ratio %.3f |" % (q, errs[q], bars[q], errs[q] / bars[q])
    print(line)
    path = os.environ.get("KRYPY_AMD_PROJ_LOG", "")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _row(hip, c, untouched=True):
    """One table row: run, compare, log, the blocks the call must leave alone; returns what the expectations need."""
    hip.set("proj_reg", 1)
    hip.set("proj_panel", 1)
    n = pc.resolve_n(c.n, hip.info()["compute_units"])
    inp = _inputs(c, n)
    ref, yard = _reference(c, n, inp)
    before = _counters(hip)
    run = pc.run_case(hip, c, inp)
    moved = tuple(a - b for a, b in zip(_counters(hip), before))
    assert (run.ya is not None) == c.want_ya
    errs, bars = pr.assert_matches((run.z, run.ya), ref, yard, c.d, pr._norm(inp.a))
    _log(c.name, n, c.d, moved, hip, errs, bars)
    if untouched:
        pc.check_untouched(c, run, blocks=n <= pc.HOST_LIMIT)
    return n, inp, run, moved


def _ids(cases):
    return [c.name for c in cases]


# ---- a. the chunked kernels (real) and e. the complex ladder ----------------------------------------------------------
@pytest.mark.parametrize("c", pc.CHUNKED + pc.COMPLEX, ids=_ids(pc.CHUNKED + pc.COMPLEX))
def test_short_vectors(hip, c):
    """k_multidot<16> / k_reduce_partials / k_small_matvec / k_multiaxpy<16> (a second chunk from d = 17, a third at 33;
    k_small_matvec's stride loop beyond d = 256; d = 1024 with 1024 numbers through the pinned staging buffer) and
    k_zmultidot / k_zsmall_matvec / k_zmultiaxpy<8, 4, 2, 1> (all four chunk widths at d = 15, d = 512; complex W, T and
    WRH: a missing or an extra conjugate shows) - neither the one-launch kernel nor the panel passes serve these."""
    n, inp, run, moved = _row(hip, c)
    expect_kernel(moved == (0, 0), "%s: one-launch / panel launches %r, expected none" % (c.name, moved))
    expect_kernel(hip.get("proj_reg_rows") == 0 and hip.get("proj_reg_why") != 0,
                  "%s: proj_reg_why %d, proj_reg_rows %d describe a one-launch projector that did not run" % (
                      c.name, hip.get("proj_reg_why"), hip.get("proj_reg_rows")))


def test_complex_limit_and_the_path_behind_it(hip):
    """513 complex vectors: kh_zproj_create refuses, and utils.Projection projects through its sweep-by-sweep path
    (dot panel, host coefficients, update panel) - compared with the reference at n = 600 like every device path."""
    from krypy_amd import _hip, utils

    n, d = 600, 513
    Wd = hip.upload(pc.block(0, n, d, True))
    with pytest.raises(_hip.BackendError):
        hip.proj_create(Wd, Wd, d, None, None, 2)
    X = pc.block(0, n, d, True) * np.sqrt(n)
    P = utils.Projection(X, iterations=2)
    assert P._device_projector() is None
    a = pc.vector(n, True)
    z, ya = P.apply_complement(a.reshape(-1, 1), return_Ya=True)
    Q, WRH = P.V, P.WR.T.conj()
    ref = pr.complement(Q, Q, d, None, WRH, 2, a)
    yard = pr.complement(Q, Q, d, None, WRH, 2, a, dtype=np.float64)
    errs, bars = pr.assert_matches((z[:, 0], ya[:, 0]), ref, yard, d, pr._norm(a))
    _log("complex-n600-d513-sweep-by-sweep", n, d, (0, 0), hip, errs, bars)


# ---- b. call forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.FORMS, ids=_ids(pc.FORMS))
def test_call_forms(hip, c):
    """In place; column 2 of three into column 1 of three; blocks two columns wider than d whose surplus columns are NaN;
    W is V.  Every other column of the target, the source, W and V bit for bit as they were, the target's padding zero;
    the same call again gives the same bits; without want_ya the same vector and nothing handed back."""
    n, inp, run, moved = _row(hip, c)
    again = pc.run_case(hip, c, inp, keep=run)
    assert pc._same_bits(again.z, run.z) and pc._same_bits(again.ya, run.ya), "the same call, other bits"
    quiet = pc.run_case(hip, c, inp, want_ya=False, keep=run)
    assert quiet.ya is None
    assert pc._same_bits(quiet.z, run.z), "without want_ya the vector differs"
    pc.check_untouched(c, quiet)
    expect_kernel(moved == (0, 0), "%s: one-launch / panel launches %r, expected none" % (c.name, moved))


# ---- c. the one-launch kernel -------------------------------------------------------------------------------------------
def _expect_reg(hip, c, n, moved):
    ncu = hip.info()["compute_units"]
    rows = pc.class_of(n, ncu)
    if SERVED:
        expect_kernel(moved[0] == 1 and hip.get("proj_reg_why") == 0 and hip.get("proj_reg_rows") == rows,
                      "%s: one-launch projector +%d (why %d, %d rows per lane), expected +1 (0, %d)" % (
                          c.name, moved[0], hip.get("proj_reg_why"), hip.get("proj_reg_rows"), rows))
        expect_kernel(moved[1] == 0, "%s: %d panel sweeps behind the one-launch kernel" % (c.name, moved[1]))
    else:      # one rank of a communicator: no grid-wide sum across GPUs, the kernel declines
        expect_kernel(moved[0] == 0 and hip.get("proj_reg_why") == 1 and hip.get("proj_reg_rows") == 0,
                      "%s: the one-launch projector ran on a communicator" % c.name)
        expect_kernel(moved[1] == (c.iterations if rows >= 40 else 0), "%s: %d panel sweeps" % (c.name, moved[1]))


@pytest.mark.parametrize("c", pc.REG, ids=_ids(pc.REG))
def test_one_launch_kernel(hip, c):
    """k_proj_reg<16 ... 56> at the smallest even n of each register shape, the 16-row shape with ncu / 2 + 1 workgroups
    (one lane in the third gather group at 256 CUs) and with all ncu full (no padding row), an odd n (the last double2
    half padding), the largest n the 56-row shape serves; at the smallest shape d = 1, 2, 8, 9 (wave 0's second value),
    15, 16 with one, two and three sweeps, in place and out of place, T without WRH and WRH without T."""
    n, inp, run, moved = _row(hip, c)
    _expect_reg(hip, c, n, moved)


def test_one_launch_kernel_sequence_of_sweep_counts(hip):
    """One, three, two, one sweeps in a row on one context: every launch starts where the epoch counter of the last one
    ended - on either granule parity, the leader stamps keyed by the first epoch of the launch.  Every result compared."""
    for i, it in enumerate((1, 3, 2, 1)):
        c = pc.case("reg-16rows-d9-sequence-%d-it%d" % (i, it), "reg", ("first", 16), 9, iterations=it, inplace=bool(i % 2))
        n, inp, run, moved = _row(hip, c, untouched=False)
        _expect_reg(hip, c, n, moved)


def test_one_launch_kernel_declines(hip):
    """d = 17 (why 1), the largest n of the 8-row shape (why 2), the switch (why 1): the other kernels serve the call and
    the numbers are right."""
    cases = [(pc.case("reg-declines-d17", "reg", ("first", 16), 17, iterations=1), 1, 1),
             (pc.case("reg-declines-8rows-last", "reg", ("last", 8), 4), 2, 1),
             (pc.case("reg-declines-switched-off", "reg", ("first", 16), 2), 1, 0)]
    for c, why, switch in cases:
        hip.set("proj_panel", 1)
        hip.set("proj_reg", switch)
        try:
            n = pc.resolve_n(c.n, hip.info()["compute_units"])
            inp = _inputs(c, n)
            ref, yard = _reference(c, n, inp)
            before = _counters(hip)
            run = pc.run_case(hip, c, inp)
            moved = tuple(a - b for a, b in zip(_counters(hip), before))
            got_why = hip.get("proj_reg_why")
            errs, bars = pr.assert_matches((run.z, run.ya), ref, yard, c.d, pr._norm(inp.a))
            _log(c.name, n, c.d, moved, hip, errs, bars)
        finally:
            hip.set("proj_reg", 1)
        expect_kernel(moved == (0, 0) and hip.get("proj_reg_rows") == 0, "%s: launches %r, expected none" % (c.name, moved))
        # (a communicator declines every call at reason 1, in front of the length)
        expect_kernel(got_why == (why if SERVED else 1), "%s: proj_reg_why %d, expected %d" % (c.name, got_why, why))


# ---- d. the panel passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.PANEL, ids=_ids(pc.PANEL))
def test_panel_passes_without_the_one_launch_kernel(hip, c):
    """cgs_panel_pass (k_cgs_dots / k_cgs_update) at the smallest n of the 40-row shape, even and odd, d = 17 - the one-launch
    kernel, left switched on, declines (d > 16) - with W is V (one block of 1.1 GB).  d > 256, where the panel passes
    decline in turn, would need a block of many GB at this length and is left out."""
    n, inp, run, moved = _row(hip, c)
    expect_kernel(moved == (0, c.iterations), "%s: one-launch / panel launches %r, expected (0, %d)" % (c.name, moved, c.iterations))


# ---- f. inside the Arnoldi step -----------------------------------------------------------------------------------------
def _operator(n, cplx):
    """Five diagonals of a 2-D Laplacian (offsets 1 and m ~ sqrt(n)) plus a small non-symmetric part."""
    m = max(2, int(np.sqrt(n)))
    rng = np.random.default_rng([n, int(cplx)])
    A = sp.diags([-1.0, -1.0, 4.0, -1.0, -1.0], [-m, -1, 0, 1, m], shape=(n, n), format="csr")
    A = A + sp.diags(0.1 * rng.standard_normal(n - 1), 1, shape=(n, n), format="csr")
    if cplx:
        A = A + 1j * sp.diags(0.1 * rng.standard_normal(n - 1), -1, shape=(n, n), format="csr")
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


_STEP = [(4099, False), (70001, False), (("first", 16), False), (4099, True)]


@pytest.mark.parametrize("d", [1, 5, 16])
@pytest.mark.parametrize("nspec,cplx", _STEP, ids=["n4099", "n70001", "16rows", "n4099-c128"])
def test_projector_inside_the_arnoldi_step(hip, nspec, cplx, d):
    """kh_arnoldi_step_begin / _end with a projector (complex: kh_zarnoldi_step_begin_proj), k = 3, one sweep: the H column,
    <Y, z_in> behind it and v_{k+1} against proj_ref.deflated_step.  4099: masked blocks and the link kernels; 70001: the
    chain kernel behind the chunked projector; the smallest 16-row n: the one-launch projector in front of it."""
    from krypy_amd import _hip

    hip.set("proj_reg", 1)
    hip.set("proj_panel", 1)
    k, its = 3, 2
    n = pc.resolve_n(nspec, hip.info()["compute_units"])
    c = pc.case("step-%s-d%d" % ("c128" if cplx else "f64", d), "step", n, d, cplx=cplx, iterations=its)
    inp = _inputs(c, n)
    A = _operator(n, cplx)
    rng = np.random.default_rng([n, 77])
    X = rng.standard_normal((n, k + 1)) + (1j * rng.standard_normal((n, k + 1)) if cplx else 0.0)
    basis = np.linalg.qr(X)[0]
    ref = pr.deflated_step(A, inp.W, inp.V, d, inp.T, inp.WRH, its, basis, k, 1)
    yard = pr.deflated_step(A, inp.W, inp.V, d, inp.T, inp.WRH, its, basis, k, 1, dtype=np.float64)
    dt = complex if cplx else float
    Vd = hip.alloc(n, k + 2, dtype=dt)
    Vd.upload(0, basis)
    Wd = hip.alloc(n, 1, dtype=dt)
    Ad = hip.csr(A)
    Bw, Bv = hip.upload(np.asarray(inp.W, dtype=dt)), hip.upload(np.asarray(inp.V, dtype=dt))
    pj = hip.proj_create(Bw, Bv, d, inp.T, inp.WRH, its)
    before = _counters(hip)
    if cplx:
        hk = np.zeros(2)
        _hip._check(hip._lib, hip._lib.kh_zarnoldi_step_begin_proj(
            hip._h, Ad.handle, pj.handle, Vd.handle, Wd.handle, 0, k, 0, 1, _hip.GS_MGS, _hip._dptr(hk), 0),
            "kh_zarnoldi_step_begin_proj")
    else:
        hip.arnoldi_step_begin(Ad, None, Vd, None, Wd, 0, k, 0, 1, _hip.GS_MGS, 0.0, 0, proj=pj)
    out = hip.arnoldi_step_end(0, k + 2 + d, cplx=cplx)
    moved = tuple(a - b for a, b in zip(_counters(hip), before))
    got = pr.DeflatedStep(out[: k + 2], out[k + 2:], Vd.download(k + 1, 1)[:, 0])
    scale = pr._norm(A.dot(basis[:, k]))
    errs, bars = pr.assert_matches(got, ref, yard, d, scale)
    _log(c.name, n, d, moved, hip, errs, bars)
    assert pc._same_bits(Vd.download(0, k + 1), np.asfortranarray(basis.astype(dt))), "the basis changed"
    assert Vd.padding_nonzero() == 0 and Wd.padding_nonzero() == 0
    long = pc.class_of(n, hip.info()["compute_units"]) >= 16 and SERVED and not cplx
    expect_kernel(moved == ((1, 0) if long else (0, 0)), "%s at n = %d: one-launch / panel launches %r" % (c.name, n, moved))


# ---- g. argument errors -------------------------------------------------------------------------------------------------
def test_argument_errors(hip):
    """A projector of the other kind, vectors of the other kind, no sweep, no column, more columns than the blocks hold:
    an error, and nothing written.  The complex blocks have m = 257 rows and the real ones n = 2 m = 514: a complex block
    IS a real block of length 2 m to the library, so every length check agrees and only the checks of the KIND stand
    between a mixed call and a launch of the real kernels over interleaved data (or the converse)."""
    from krypy_amd import _hip

    m, d, k = 257, 3, 1
    n = 2 * m
    real = hip.upload(pc.block(0, n, d, False))
    cplx = hip.upload(pc.block(0, m, d, True))
    assert real.ld == cplx.ld      # (the same kh_vec shape)
    pr_ = hip.proj_create(real, real, d, pc.small(2, d, False), pc.small(3, d, False), 2)
    pz = hip.proj_create(cplx, cplx, d, pc.small(2, d, True), pc.small(3, d, True), 2)
    a_r, a_z = pc.vector(n, False), pc.vector(m, True)
    Ar, Az = hip.upload(a_r), hip.upload(a_z)
    Zr, Zz = hip.upload(a_r[::-1].copy()), hip.upload(a_z[::-1].copy())
    Opr, Opz = hip.csr(_operator(n, False)), hip.csr(_operator(m, True))
    Vr, Vz = hip.alloc(n, k + 2), hip.alloc(m, k + 2, dtype=complex)
    Vr.upload(0, np.linalg.qr(pc.block(1, n, k + 1, False))[0])
    Vz.upload(0, np.linalg.qr(pc.block(1, m, k + 1, True))[0])
    Wr, Wz = hip.alloc(n, 1), hip.alloc(m, 1, dtype=complex)
    hk = np.zeros(2)
    lib, h = hip._lib, hip._h

    def c_call(fn, *args):
        _hip._check(lib, fn(h, *args), "call")

    wrong = [
        lambda: c_call(lib.kh_proj_apply_complement, pz.handle, Ar.handle, 0, Zr.handle, 0, None),
        lambda: c_call(lib.kh_zproj_apply_complement, pr_.handle, Az.handle, 0, Zz.handle, 0, None),
        lambda: hip.arnoldi_step_begin(Opr, None, Vr, None, Wr, 0, k, 0, 1, _hip.GS_MGS, 0.0, 0, proj=pz),
        lambda: hip.arnoldi_step_begin(Opz, None, Vz, None, Wz, 0, k, 0, 1, _hip.GS_MGS, 0.0, 0, proj=pr_),
        lambda: c_call(lib.kh_zarnoldi_step_begin_proj, Opz.handle, pr_.handle, Vz.handle, Wz.handle, 0, k, 0, 1,
                       _hip.GS_MGS, _hip._dptr(hk), 0),
        lambda: hip.proj_apply_complement(pr_, Az, 0, Zz, 0),
        lambda: hip.proj_apply_complement(pr_, Ar, 0, Zz, 0),
        lambda: hip.proj_apply_complement(pr_, Az, 0, Zr, 0),
        lambda: hip.proj_apply_complement(pz, Ar, 0, Zr, 0),
        lambda: hip.proj_apply_complement(pz, Az, 0, Zr, 0),
        lambda: hip.proj_apply_complement(pr_, Az, 0, Zz, 0, want_ya=True),
        lambda: hip.proj_apply_complement(pz, Ar, 0, Zr, 0, want_ya=True),
        lambda: hip.proj_create(real, real, d, None, None, 0),
        lambda: hip.proj_create(cplx, cplx, d, None, None, 0),
        lambda: hip.proj_create(real, real, 0, None, None, 2),
        lambda: hip.proj_create(cplx, cplx, 0, None, None, 2),
        lambda: hip.proj_create(real, real, d + 1, None, None, 2),
        lambda: hip.proj_create(cplx, cplx, d + 1, None, None, 2),
        lambda: hip.proj_create(real, cplx, d, None, None, 2),
    ]
    before = _counters(hip)
    for i, call in enumerate(wrong):
        with pytest.raises(_hip.BackendError):
            call()
            pytest.fail("call %d went through" % i)
    assert _counters(hip) == before
    # nothing was written: the targets, the step's vectors and the new basis column are what they were
    assert pc._same_bits(Zr.download()[:, 0], a_r[::-1].copy()) and pc._same_bits(Zz.download()[:, 0], a_z[::-1].copy())
    for blk in (Wr, Wz):
        assert not np.any(blk.download())
    assert not np.any(Vr.download(k + 1, 1)) and not np.any(Vz.download(k + 1, 1))
    # and the projectors still work
    for pj, A_, Z_, a_, W_ in ((pr_, Ar, Zr, a_r, real), (pz, Az, Zz, a_z, cplx)):
        ya = hip.proj_apply_complement(pj, A_, 0, Z_, 0, want_ya=True)
        Wh, ck = W_.download(), a_.dtype.kind == "c"
        ref = pr.complement(Wh, Wh, d, pc.small(2, d, ck), pc.small(3, d, ck), 2, a_)
        yard = pr.complement(Wh, Wh, d, pc.small(2, d, ck), pc.small(3, d, ck), 2, a_, dtype=np.float64)
        pr.assert_matches((Z_.download()[:, 0], ya), ref, yard, d, pr._norm(a_))
