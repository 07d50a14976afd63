"""k_mgs_chain_lds where a part of every column comes back from memory for the update (krypy_amd/csrc/chain.h, NG > 0: 24, 32 and
40 rows per lane): the dot phase ends with its last TWO batches in the register ring, the update phase consumes both, requests the
batches between them and the parked rows two at a time and leaves the next column's first batch in ring[0] for the next link (or
for nobody, behind the last one).  Which slot a batch sits in changes no operand: every row of w is updated once per link with the
same alpha and the same column entry, and the dot adds its rows in ascending order.  So H and the basis must have the bits of the
plain kernel k_mgs_chain (``chain_lds = 0``), whose arithmetic is the same and whose ring has no such schedule.

Sizes (256 compute units): the smallest vectors of each class, just above 2 * R2_prev * 512 * ncu rows - 4,194,304 / 6,291,456 /
8,388,608 for 24 / 32 / 40 rows per lane; a complex vector has one double2 row per entry, so half as many entries.  The "odd"
operator has an odd row count: the last workgroup with rows is partly padding and row n shares a 16-byte row with row n - 1.

Steps of a sequence: k = 0 .. 4, so 1 .. 5 links per launch (the ring's state goes from link to link and from the last link into
the norm), step 3 with two sweeps (8 links, every column twice), step 4 Lanczos-style (one link behind the pre-subtraction of
h v_3).  The operator runs in the prologue - mask form through the LDS window (the Laplacian), value copy through the gathers (the
"odd" operator), the complex copy - or as a launch of its own (``chain_spmv = 0``)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as ref
from tests.support import poison as po
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

M = 5                    # Arnoldi steps of a sequence
DOUBLE_SWEEP_AT = 3      # ... this one with two sweeps
LANCZOS_AT = 4           # ... and this one Lanczos-style: start = k, w -= h_{k,k-1} v_{k-1} in front of the one link
# |H - H_ref| <= 1e-12 |H_ref|, for all of H and for each of its columns by itself: the bar of
# test_mgs_chain_every_register_shape, which tests/test_gpu_poison.py holds this kernel family to against the same reference (_BAR5)
H_BAR = 1e-12

_BELOW = {24: 16, 32: 24, 40: 32}      # the class below


def _limit(ctx, rows, cplx):
    """Vectors with more entries than this take more than `rows` rows per lane."""
    return 2 * rows * 512 * ctx.info()["compute_units"] // (2 if cplx else 1)


@functools.lru_cache(maxsize=2)
def _operator(kind, lo):
    """Built once per size (consecutive cases share it)."""
    if kind in ("lap2d", "zlap2d"):        # 5 diagonals, constant coefficients: the mask form of the banded copy (real)
        nx = 1000
        A = ref.laplace2d(nx, lo // nx + 1)
        if kind == "zlap2d":
            A = (A + 0.3j * sp.diags(np.random.default_rng(6).standard_normal(A.shape[0]))).tocsr()
        return A
    # "odd" of tests/test_gpu_chain_park.py: odd row count, five diagonals with values of their own (the value copy)
    n = lo + 3
    rng = np.random.default_rng(17)
    offsets = (-3000, -1, 0, 2, 2999)
    diags = []
    for o in offsets:
        d = rng.standard_normal(n - abs(o))
        d[d == 0.0] = 1.0
        diags.append(d)
    A = sp.diags(diags, offsets, shape=(n, n)).tocsr()
    A.sort_indices()
    return A


def _start_vector(n, cplx):
    rng = np.random.default_rng(40)
    v = rng.standard_normal(n)
    if cplx:
        v = v + 1j * rng.standard_normal(n)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=2)
def _reference(kind, lo):
    """H of the whole sequence in extended precision; computed once per operator and shared by the cases on it.  The Arnoldi
    steps in front of the Lanczos-style one (the two-sweep step among them) are arnoldi_longdouble's; the last column is that
    step written out on the reference's own basis: w = A v_k - h_{k,k-1} v_{k-1}, one link against v_k, the norm."""
    A = _operator(kind, lo)
    v = _start_vector(A.shape[0], kind == "zlap2d")
    k = LANCZOS_AT
    assert k == M - 1 and DOUBLE_SWEEP_AT < k
    Ha, V, _ = po.arnoldi_longdouble(A, v, k, [2 if j == DOUBLE_SWEEP_AT else 1 for j in range(k)])
    H = np.zeros((M + 1, M), dtype=Ha.dtype)
    H[: k + 1, : k] = Ha
    w = po._apply_by_diagonals(A, V[:, k])
    w -= H[k, k - 1] * V[:, k - 1]
    alpha = np.vdot(V[:, k], w)
    w -= alpha * V[:, k]
    H[k, k] = alpha
    H[k + 1, k] = np.sqrt(np.vdot(w, w).real)
    H.setflags(write=False)
    return H


def _sequence(ctx, A, v, chain_lds, chain_spmv, poisoned):
    """M steps through kh_arnoldi_step, every one a chain launch with at least one link (the three-pass Lanczos kernel, which
    would take the one-link steps, is switched off; so is k_mgs_chain_pf, which would take the 24-row shape)."""
    n = A.shape[0]
    dt = complex if np.iscomplexobj(v) else float
    pf0 = ctx.get("chain_pf")
    ctx.set("chain_lds", chain_lds)
    ctx.set("chain_spmv", chain_spmv)
    ctx.set("lanczos_fused", 0)
    ctx.set("chain_pf", 0)
    try:
        Ad = ctx.csr(A)
        V, W = ctx.alloc(n, M + 2, dtype=dt), ctx.alloc(n, 2, dtype=dt)      # one column more than the sequence writes
        if poisoned:
            po.poison(V)
            po.poison(W)
        V.upload(0, v)
        c0 = dict(ctx.counters())
        x0, m0, p0 = ctx.get("n_chain_xwin"), ctx.get("n_dia_mask"), ctx.get("n_chain_pf")
        H = np.zeros((M + 1, M), dtype=dt)
        for k in range(M):
            lanczos = k == LANCZOS_AT
            start = k if lanczos else 0
            hk = float(H[k, k - 1].real) if lanczos else 0.0
            hcol = ctx.arnoldi_step(Ad, None, V, None, W, 0, k, start, 2 if k == DOUBLE_SWEEP_AT else 1, 0, hk)
            H[start: k + 2, k] = hcol[start: k + 2]
        c1 = dict(ctx.counters())
        used = {key: c1[key] - c0[key] for key in c1}
        used["xwin"] = ctx.get("n_chain_xwin") - x0
        used["dia_mask"] = ctx.get("n_dia_mask") - m0
        used["chain_pf"] = ctx.get("n_chain_pf") - p0
        return dict(H=H, V=V.download(0, M + 1), pad=(V.padding_nonzero(), W.padding_nonzero()), used=used)
    finally:
        ctx.set("chain_lds", 1)
        ctx.set("chain_spmv", 1)
        ctx.set("lanczos_fused", 1)
        ctx.set("chain_pf", pf0)


# (rows per lane, operator, chain_spmv); consecutive cases share an operator and its reference
_CASES = [(24, "lap2d", 1), (24, "lap2d", 0), (24, "odd", 1), (24, "zlap2d", 1),
          (32, "lap2d", 1), (32, "lap2d", 0), (32, "odd", 1), (32, "zlap2d", 1),
          (40, "lap2d", 1), (40, "lap2d", 0), (40, "odd", 1), (40, "odd", 0), (40, "zlap2d", 1), (40, "zlap2d", 0)]


@pytest.mark.parametrize("rows,kind,chain_spmv", _CASES)
def test_two_batches_held_give_the_bits_of_the_plain_kernel(hip, rows, kind, chain_spmv):
    """Five steps with k_mgs_chain_lds, with the plain kernel (chain_lds = 0) and with k_mgs_chain_lds on blocks that are NaN in
    every column, one more than is ever written: H and all of V bit for bit, the padding of V and W still zero, all of H - the
    two-sweep and the Lanczos-style column too - against the extended-precision reference."""
    cplx = kind == "zlap2d"
    lo, hi = _limit(hip, _BELOW[rows], cplx), _limit(hip, rows, cplx)
    A = _operator(kind, lo)
    n = A.shape[0]
    assert lo < n <= hi, "the size must take the %d-row shape: %r" % (rows, (lo, n, hi))
    v = _start_vector(n, cplx)
    lds = _sequence(hip, A, v, 1, chain_spmv, False)
    plain = _sequence(hip, A, v, 0, chain_spmv, False)
    po.bits_equal(lds["H"], plain["H"], "H, k_mgs_chain_lds against the plain kernel")
    po.bits_equal(lds["V"], plain["V"], "V, k_mgs_chain_lds against the plain kernel")
    del plain["V"]
    nan = _sequence(hip, A, v, 1, chain_spmv, True)
    po.bits_equal(nan["H"], lds["H"], "H on poisoned blocks")
    po.bits_equal(nan["V"], lds["V"], "V on poisoned blocks")
    del nan["V"]
    assert np.all(np.isfinite(lds["H"])) and np.all(np.isfinite(lds["V"]))
    for name, run in (("lds", lds), ("plain", plain), ("poisoned", nan)):
        assert run["pad"] == (0, 0), "non-zero padding words of (V, W), %s run: %r" % (name, run["pad"])
    Href = _reference(kind, lo)
    assert Href.shape == lds["H"].shape
    diff = (lds["H"] - Href).astype(complex)
    herr, href = float(np.linalg.norm(diff)), float(np.linalg.norm(Href.astype(complex)))
    cols = [float(np.linalg.norm(diff[:, k])) / float(np.linalg.norm(Href[:, k].astype(complex))) for k in range(M)]
    print("FIGURES hold2-%d-%s-%d: |H - H_ref| / |H_ref| = %.3e, by column (3: two sweeps, 4: Lanczos-style) %s (bar %.0e)"
          % (rows, kind, chain_spmv, herr / href, " ".join("%.2e" % c for c in cols), H_BAR))
    assert herr <= H_BAR * href, (herr / href, H_BAR)
    assert max(cols) <= H_BAR, (cols, H_BAR)
    # which kernels ran (judged after the comparisons)
    for name, run, want in (("lds", lds, M), ("plain", plain, 0), ("poisoned", nan, M)):
        expect_kernel(run["used"]["chain"] == M and run["used"]["chain_lds"] == want and run["used"]["chain_pf"] == 0,
                      "%s run: %d chain launches, %d of them k_mgs_chain_lds: %r" % (name, M, want, run["used"]))
        expect_kernel(run["used"]["chain_fused"] == (M if chain_spmv else 0),
                      "%s run: operator in the prologue %d times: %r" % (name, M if chain_spmv else 0, run["used"]))
    # the form of the prologue: the Laplacian's masks through the window, the value copy (and the complex one) through gathers
    for name, run in (("lds", lds), ("poisoned", nan)):
        expect_kernel(run["used"]["xwin"] == (M if (kind == "lap2d" and chain_spmv) else 0),
                      "%s run: launches through the x window: %r" % (name, run["used"]))
    if chain_spmv:
        expect_kernel((lds["used"]["dia_mask"] >= M) == (kind == "lap2d"), "mask form: %r" % (lds["used"],))
