"""k_mgs_chain_lds at 40 rows per lane (krypy_amd/csrc/chain.h): 19 of a column's 40 double2 rows are parked in LDS between
its dot and its update, the fourth batch is split (rows 15..18 parked, row 19 read again alone) and, with the operator in the
prologue, the last four rows of w wait in LDS until the prologue's registers are free.  Arithmetic and its order are those of the
plain kernel k_mgs_chain<40>, so the bits are too.

Sizes: the smallest vectors that take the 40-row shape, just above the 32-row limit 2 * 32 * 512 * ncu (8,388,608 rows on 256
compute units: 2900 x 2900, 204^3, and the limit + 3 as an odd size).  206 of the workgroups carry rows, the last one partly
padding."""
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
DOUBLE_SWEEP_AT = 3      # ... this one with two sweeps (every parked row is overwritten per link, LDS holds another column)
LANCZOS_AT = 4           # ... and this one Lanczos-style: start = k, w -= h_{k-1,k} v_{k-1} in front of the one link


def _limits(ctx):
    ncu = ctx.info()["compute_units"]
    return 2 * 32 * 512 * ncu, 2 * 40 * 512 * ncu


@functools.lru_cache(maxsize=3)
def _operator(kind, lo):
    """Built once per size."""
    if kind == "lap2d":                    # 5 diagonals, constant coefficients: the mask form of the banded copy
        nx = 100 * (int(np.sqrt(lo)) // 100 + 1)
        return ref.laplace2d(nx, nx)
    if kind == "lap3d":                    # 7 diagonals
        nx = int(np.ceil(np.cbrt(lo + 1)))
        return ref.laplace3d(nx).tocsr()
    # odd row count, 5 diagonals with values of their own (the value copy), odd and even offsets, not symmetric
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


def _sequence(ctx, A, v, chain_lds, chain_spmv, poisoned):
    """M steps through kh_arnoldi_step; every one of them is a chain launch with at least one link in k_mgs_chain_lds<40> /
    k_mgs_chain<40> (the three-pass Lanczos kernel, which would take the one-link steps, is switched off)."""
    n = A.shape[0]
    ctx.set("chain_lds", chain_lds)
    ctx.set("chain_spmv", chain_spmv)
    ctx.set("lanczos_fused", 0)
    try:
        Ad = ctx.csr(A)
        V, W = ctx.alloc(n, M + 2), ctx.alloc(n, 2)      # one column more than the sequence writes
        if poisoned:
            po.poison(V)
            po.poison(W)
        V.upload(0, v)
        c0 = ctx.counters()
        H = np.zeros((M + 1, M))
        for k in range(M):
            lanczos = k == LANCZOS_AT
            start = k if lanczos else 0
            hk = float(H[k, k - 1]) if lanczos else 0.0
            hcol = ctx.arnoldi_step(Ad, None, V, None, W, 0, k, start, 2 if k == DOUBLE_SWEEP_AT else 1, 0, hk)
            H[start: k + 2, k] = hcol[start: k + 2]
        c1 = ctx.counters()
        used = {key: c1[key] - c0[key] for key in c1}
        return dict(H=H, V=V.download(0, M + 1), pad=(V.padding_nonzero(), W.padding_nonzero()), used=used,
                    diagonals=Ad.diagonals)
    finally:
        ctx.set("chain_lds", 1)
        ctx.set("chain_spmv", 1)
        ctx.set("lanczos_fused", 1)


@pytest.mark.parametrize("kind,chain_spmv", [("lap2d", 1), ("lap2d", 0), ("lap3d", 1), ("lap3d", 0), ("odd", 1), ("odd", 0)])
def test_parked_rows_give_the_bits_of_the_plain_kernel(hip, kind, chain_spmv):
    """Five steps (one double-sweep, one Lanczos-style with its pre-subtraction) with the LDS kernel, with the plain kernel
    (chain_lds = 0) and with the LDS kernel on blocks that are NaN in every column, one more than is ever written: H and all
    of V bit for bit, the padding of V and W still zero.  With chain_spmv = 1 the operator runs in the prologue (mask form for
    the Laplacians, value copy for the odd size), with 0 as a launch of its own."""
    lo, hi = _limits(hip)
    A = _operator(kind, lo)
    n = A.shape[0]
    assert lo < n <= hi, "the size must take the 40-row shape: %r" % ((lo, n, hi),)
    v = np.random.default_rng(40).standard_normal(n)
    v /= np.linalg.norm(v)
    lds = _sequence(hip, A, v, 1, chain_spmv, False)
    plain = _sequence(hip, A, v, 0, chain_spmv, False)
    po.bits_equal(lds["H"], plain["H"], "H, parked rows against the plain kernel")
    po.bits_equal(lds["V"], plain["V"], "V, parked rows against the plain kernel")
    del plain["V"]
    nan = _sequence(hip, A, v, 1, chain_spmv, True)
    po.bits_equal(nan["H"], lds["H"], "H on poisoned blocks")
    po.bits_equal(nan["V"], lds["V"], "V on poisoned blocks")
    assert np.all(np.isfinite(lds["H"])) and np.all(np.isfinite(lds["V"]))
    for name, run in (("parked", lds), ("plain", plain), ("poisoned", nan)):
        assert run["pad"] == (0, 0), "non-zero padding words of (V, W), %s run: %r" % (name, run["pad"])
    # which kernels ran (judged after the comparisons)
    expect_kernel(lds["diagonals"] in (5, 7), "the operator has its banded copy: %r" % (lds["diagonals"],))
    for name, run, want in (("parked", lds, M), ("plain", plain, 0), ("poisoned", nan, M)):
        expect_kernel(run["used"]["chain"] == M and run["used"]["chain_lds"] == want,
                      "%s run: %d chain launches, %d of them with parked rows: %r" % (name, M, want, run["used"]))
        expect_kernel(run["used"]["chain_fused"] == (M if chain_spmv else 0),
                      "%s run: operator in the prologue %d times: %r" % (name, M if chain_spmv else 0, run["used"]))


def test_timeout_at_40_rows_is_recovered(hip):
    """kh_ctx_set("chain_fault", 1): the next chain launch reports a timed-out sum and leaves halved coefficients behind.  At
    the 2-D size the step is run again on the per-column kernels from the intact columns; the residual history of the solve
    after it is that of the undisturbed one, as tests/test_gpu_parity.py::test_chain_timeout_is_recovered has it at its sizes
    (the faulted solve itself sums in another order from the fault on: same length, equal to rounding)."""
    lo, hi = _limits(hip)
    A = _operator("lap2d", lo)
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

        before, lds0 = hip.get("n_chain_recovered"), hip.counters()["chain_lds"]
        try:
            sol = Faulty(ls, **kw)
        except utils.ConvergenceError as e:
            sol = e.solver
        return np.asarray(sol.resnorms), hip.get("n_chain_recovered") - before, hip.counters()["chain_lds"] - lds0

    try:
        good, n0, lds_good = run(-1)
        bad, n1, _ = run(2)
        off_after = hip.get("chain")
        again, n2, lds_again = run(-1, reset=False)
    finally:
        hip.set("chain_fault", 0)
        hip.set("chain", 1)
    po.bits_equal(again, good, "residual history after the recovery against the undisturbed run")
    assert len(bad) == len(good) == kw["maxiter"] + 1
    # the re-run step sums its inner products in another order: rounding of sums over 8.4 M terms, far below 1e-10
    assert np.allclose(bad, good, rtol=1e-10, atol=0.0), np.max(np.abs(bad - good) / good)
    expect_kernel(n0 == 0 and n1 >= 1 and n2 == 0, "recoveries clean / faulted / next run: %r" % ((n0, n1, n2),))
    expect_kernel(off_after == 0 and hip.get("chain") == 1, "chain off after the timeout, on again with the next basis")
    expect_kernel(lds_good >= kw["maxiter"] - 1 and lds_again == lds_good,
                  "launches with parked rows, undisturbed / after the recovery: %r" % ((lds_good, lds_again),))
