"""The x window of k_mgs_chain_lds' operator prologue (krypy_amd/csrc/chain.h: chain_apply_banded_xwin).

With a constant-coefficient banded operator (mask form) the workgroup copies its stretch of x block by block into a ring of LDS
blocks - the parked rows, idle during the prologue - and the lanes take a row pair's neighbour values from there instead of
through clamped global gathers.  The same values of x enter the same operations in the same order, so H and the basis must be
bit for bit those of the gathers (``chain_xwin = 0``) and of the separate SpMV launch (``chain_spmv = 0``).  A ring block is the
1024 doubles of one row of the chunk; the window is taken when the blocks a row reads from, and the one staged beside them, fit
the ring: 15 blocks at 40 rows per lane, 12 at 16 ... 32.  ``n_chain_xwin`` counts the launches that took it.

Sizes (256 compute units): the smallest vectors of the 40-row class, just above 2 * 32 * 512 * ncu = 8,388,608 rows - the first
workgroup's window reaches before row 0, the last workgroup with rows is partly padding - and of the 16-row class, the smallest
one the prologue is instantiated for."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from krypy_amd import linsys, utils
from oracle import krylov_ref as ref
from tests.support import poison as po
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

M = 5                    # Arnoldi steps of a sequence
DOUBLE_SWEEP_AT = 3      # ... this one with two sweeps
LANCZOS_AT = 4           # ... and this one Lanczos-style: start = k, w -= h_{k-1,k} v_{k-1} in front of the one link


def _limit(ctx, rows):
    """Vectors longer than this take more than `rows` rows per lane."""
    return 2 * rows * 512 * ctx.info()["compute_units"]


def _grid(nx, lo):
    """nx x ny grid with the fewest rows above lo."""
    return ref.laplace2d(nx, lo // nx + 1)


@functools.lru_cache(maxsize=2)
def _operator(kind, lo):
    """(operator, mask form expected, window expected); built once per size."""
    if kind == "lap2d":                    # offsets +-2900: 3 blocks before and behind a row's own
        nx = 100 * (int(np.sqrt(lo)) // 100 + 1)
        return ref.laplace2d(nx, nx), True, True
    if kind == "holes":
        # odd row count; constant coefficients, offsets that are not symmetric, odd and even ones, and an irregular mask: a few
        # percent of the entries removed (tests/test_gpu_dia_mask.py: "holes"), every diagonal still more than 70 % full
        n = lo + 3
        offsets = (-3001, -2, 0, 1, 2999)
        values = (-1.25, 0.5, 4.0, -0.75, -1.5)
        A = sp.diags([np.full(n - abs(o), c) for o, c in zip(offsets, values)], offsets, shape=(n, n)).tocoo()
        keep = np.random.default_rng(5).random(A.nnz) > 0.04
        A = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=A.shape)
        A.sort_indices()
        return A, True, True
    if kind == "nx6144":                   # 6 + 1 + 6 blocks read, one staged: 14 of the ring's 15 - the widest band that fits
        return _grid(6144, lo), True, True
    if kind == "nx6145":                   # one column more: 7 + 1 + 7 blocks and no room to stage into
        return _grid(6145, lo), True, False
    if kind == "nx8400":                   # a span of 16,800 doubles, more than the ring holds
        return _grid(8400, lo), True, False
    if kind == "rows16":
        return _grid(1500, lo), True, True
    # "odd" of tests/test_gpu_chain_park.py: five diagonals with values of their own - the value copy, no window
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
    return A, False, False


def _sequence(ctx, A, v, chain_xwin, chain_spmv, poisoned, chain_pf):
    """M steps through kh_arnoldi_step, every one a launch of k_mgs_chain_lds with at least one link (the three-pass Lanczos
    kernel, which would take the one-link steps, is switched off; so is k_mgs_chain_pf where it would take the shape)."""
    n = A.shape[0]
    ctx.set("chain_xwin", chain_xwin)
    ctx.set("chain_spmv", chain_spmv)
    ctx.set("lanczos_fused", 0)
    pf0 = ctx.get("chain_pf")
    ctx.set("chain_pf", chain_pf)
    try:
        Ad = ctx.csr(A)
        V, W = ctx.alloc(n, M + 2), ctx.alloc(n, 2)      # one column more than the sequence writes
        if poisoned:
            po.poison(V)
            po.poison(W)
        V.upload(0, v)
        c0 = ctx.counters()
        x0, m0 = ctx.get("n_chain_xwin"), ctx.get("n_dia_mask")
        H = np.zeros((M + 1, M))
        for k in range(M):
            lanczos = k == LANCZOS_AT
            start = k if lanczos else 0
            hk = float(H[k, k - 1]) if lanczos else 0.0
            hcol = ctx.arnoldi_step(Ad, None, V, None, W, 0, k, start, 2 if k == DOUBLE_SWEEP_AT else 1, 0, hk)
            H[start: k + 2, k] = hcol[start: k + 2]
        c1 = ctx.counters()
        used = {key: c1[key] - c0[key] for key in c1}
        used["xwin"] = ctx.get("n_chain_xwin") - x0
        used["dia_mask"] = ctx.get("n_dia_mask") - m0
        return dict(H=H, V=V.download(0, M + 1), pad=(V.padding_nonzero(), W.padding_nonzero()), used=used,
                    diagonals=Ad.diagonals)
    finally:
        ctx.set("chain_xwin", 1)
        ctx.set("chain_spmv", 1)
        ctx.set("lanczos_fused", 1)
        ctx.set("chain_pf", pf0)


# (kind, rows per lane of the class below the one under test, rows per lane under test)
_CASES = [("lap2d", 32, 40), ("holes", 32, 40), ("nx6144", 32, 40), ("nx6145", 32, 40), ("nx8400", 32, 40), ("rows16", 8, 16),
          ("odd", 32, 40)]


@pytest.mark.parametrize("kind,below,rows", _CASES)
def test_window_gives_the_bits_of_the_gathers(hip, kind, below, rows):
    """Five steps (one double-sweep, one Lanczos-style with its pre-subtraction) with the window, with the gathers
    (chain_xwin = 0) and with the operator as a launch of its own (chain_spmv = 0): H and all of V bit for bit; the same bits
    again on blocks that are NaN in every column; the padding of V and W still zero; the window's counter moved by exactly the
    launches of the window run where the band fits the ring, and not at all otherwise."""
    lo, hi = _limit(hip, below), _limit(hip, rows)
    A, masked, fits = _operator(kind, lo)
    n = A.shape[0]
    assert lo < n <= hi, "the size must take the %d-row shape: %r" % (rows, (lo, n, hi))
    pf = 0 if rows <= 24 else hip.get("chain_pf")      # (up to 24 rows per lane k_mgs_chain_pf would take the step)
    v = np.random.default_rng(40).standard_normal(n)
    v /= np.linalg.norm(v)
    win = _sequence(hip, A, v, 1, 1, False, pf)
    gat = _sequence(hip, A, v, 0, 1, False, pf)
    po.bits_equal(win["H"], gat["H"], "H, window against gathers")
    po.bits_equal(win["V"], gat["V"], "V, window against gathers")
    del gat["V"]
    sep = _sequence(hip, A, v, 1, 0, False, pf)
    po.bits_equal(win["H"], sep["H"], "H, window against the separate SpMV launch")
    po.bits_equal(win["V"], sep["V"], "V, window against the separate SpMV launch")
    del sep["V"]
    nan = _sequence(hip, A, v, 1, 1, True, pf)
    po.bits_equal(nan["H"], win["H"], "H on poisoned blocks")
    po.bits_equal(nan["V"], win["V"], "V on poisoned blocks")
    assert np.all(np.isfinite(win["H"])) and np.all(np.isfinite(win["V"]))
    for name, run in (("window", win), ("gathers", gat), ("separate", sep), ("poisoned", nan)):
        assert run["pad"] == (0, 0), "non-zero padding words of (V, W), %s run: %r" % (name, run["pad"])
    # which kernels ran (judged after the comparisons)
    expect_kernel(win["diagonals"] == 5, "the operator has its banded copy: %r" % (win["diagonals"],))
    for name, run, fused in (("window", win, M), ("gathers", gat, M), ("separate", sep, 0), ("poisoned", nan, M)):
        expect_kernel(run["used"]["chain"] == M and run["used"]["chain_lds"] == M and run["used"]["chain_fused"] == fused,
                      "%s run: %d launches of k_mgs_chain_lds, %d with the operator in the prologue: %r" % (name, M, fused, run["used"]))
    expect_kernel((win["used"]["dia_mask"] >= M) == masked, "mask form: %r, %r" % (masked, win["used"]))
    want = M if fits else 0
    expect_kernel(win["used"]["xwin"] == want and nan["used"]["xwin"] == want,
                  "launches through the window: %d expected: %r, %r" % (want, win["used"], nan["used"]))
    expect_kernel(gat["used"]["xwin"] == 0 and sep["used"]["xwin"] == 0,
                  "no window with chain_xwin = 0 / chain_spmv = 0: %r, %r" % (gat["used"], sep["used"]))


def test_timeout_with_the_window_is_recovered(hip):
    """kh_ctx_set("chain_fault", 1) during a whole Gmres solve whose steps read x through the window: the step is run again on
    the per-column kernels from the intact columns, and the solve after it has the residual history of the undisturbed one - as
    tests/test_gpu_chain_park.py::test_timeout_at_40_rows_is_recovered has it for the gathers."""
    lo = _limit(hip, 32)
    A = _operator("lap2d", lo)[0]
    n = A.shape[0]
    b = np.random.default_rng(5).standard_normal(n)
    kw = dict(maxiter=6, tol=1e-30)

    def run(fault_at, reset=True):
        if reset:
            hip.set("chain", 1)
        ls = linsys.LinearSystem(A, b)

        class Faulty(linsys.Gmres):
            def _finalize_iteration(self, yk, resnorm):
                if self.iter == fault_at:
                    hip.set("chain_fault", 1)
                return super(Faulty, self)._finalize_iteration(yk, resnorm)

        before, x0 = hip.get("n_chain_recovered"), hip.get("n_chain_xwin")
        try:
            sol = Faulty(ls, **kw)
        except utils.ConvergenceError as e:
            sol = e.solver
        return np.asarray(sol.resnorms), hip.get("n_chain_recovered") - before, hip.get("n_chain_xwin") - x0

    try:
        good, n0, x_good = run(-1)
        bad, n1, _ = run(2)
        off_after = hip.get("chain")
        again, n2, x_again = run(-1, reset=False)
    finally:
        hip.set("chain_fault", 0)
        hip.set("chain", 1)
    po.bits_equal(again, good, "residual history after the recovery against the undisturbed run")
    assert len(bad) == len(good) == kw["maxiter"] + 1
    # the re-run step sums its inner products in another order: rounding of sums over 8.4 M terms, far below 1e-10
    assert np.allclose(bad, good, rtol=1e-10, atol=0.0), np.max(np.abs(bad - good) / good)
    expect_kernel(n0 == 0 and n1 >= 1 and n2 == 0, "recoveries clean / faulted / next run: %r" % ((n0, n1, n2),))
    expect_kernel(off_after == 0 and hip.get("chain") == 1, "chain off after the timeout, on again with the next basis")
    expect_kernel(x_good >= kw["maxiter"] - 1 and x_again == x_good,
                  "launches through the window, undisturbed / after the recovery: %r" % ((x_good, x_again),))
