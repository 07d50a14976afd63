"""Measurements of the Chebyshev polynomial preconditioner (krypy_amd/csrc/cheb.hip) for KERNELS.md; not part of bench.py.

    python tools/cheb_bench.py [--what kernels,solve] [--big 1] [--reps 20] [--cap 20000]

kernels  time per application ``z = p(A) r`` at degree 4 and 8 on the five-point Laplacian (mask form) at N = 10^6 (and 10^7 with
         --big 1) and on a random symmetric matrix of ~7 entries per row (CSR-stream) at N = 10^6: the fused epilogue against
         the composed path (kh_apply + k_cheb_update) against m - 1 plain kh_apply calls, the three alternating within one
         process, device events around `reps` back-to-back applications after a warm-up, median of 5 rounds.
solve    time to tol 1e-8 - wall clock around the solver call, the device drained - on the 4000 x 2500 Laplacian (1000 x 1000
         without --big 1): CG and restarted GMRES(100), each plain, with the Jacobi diagonal, and with chebyshev_operator at
         degree 4 and 8 (defaults otherwise), with the iteration counts.  --cap bounds the iterations of one run; a run that
         stops there is reported with converged = false.
Every line printed is one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support import cheb_cases as cc      # noqa: E402  (the matrices of the tests)


def timed(ctx, fn, reps):
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def bench_kernels(ctx, name, A, lmax, reps, rounds=5):
    from krypy_amd.utils import chebyshev_coefficients

    n = A.shape[0]
    dm = ctx.csr(A)
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y, S = ctx.alloc(n, 1), ctx.alloc(n, 3)
    m0 = ctx.get("n_dia_mask")
    ctx.apply(dm, X, 0, Y, 0, 1)
    form = "csr-stream" if not dm.diagonals else ("banded, mask form" if ctx.get("n_dia_mask") > m0 else "banded, value form")
    for m in (4, 8):
        coef = chebyshev_coefficients(lmax / 30.0, lmax, m)

        def fused():
            ctx.set("cheb_fused", 1)
            ctx.cheb_apply(dm, None, coef, X, 0, Y, 0, 1, S)

        def composed():
            ctx.set("cheb_fused", 0)
            ctx.cheb_apply(dm, None, coef, X, 0, Y, 0, 1, S)

        def spmvs():
            for k in range(m - 1):
                ctx.apply(dm, S if k % 2 else X, 1 if k % 2 else 0, S, 2 if k % 2 else 1, 1)

        variants = (("fused", fused), ("composed", composed), ("spmv_only", spmvs))
        for _, fn in variants:
            fn()
        ms = {k: [] for k, _ in variants}
        for _ in range(rounds):
            for k, fn in variants:
                ms[k].append(timed(ctx, fn, reps))
        ctx.set("cheb_fused", 1)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        # vector traffic per step k >= 1: fused reads z, r, d and writes d, z'; composed writes and reads A z and streams r, d, z, d, z'
        print(json.dumps(dict(what="kernels", operator=name, n=n, nnz=int(A.nnz), diagonals=dm.diagonals, form=form, degree=m,
                              ms=med, all_ms=ms, fused_over_composed=med["fused"] / med["composed"],
                              fused_over_spmv_only=med["fused"] / med["spmv_only"],
                              us_per_fused_step=1e3 * med["fused"] / m, vector_bytes_model=dict(fused=40 * n, composed=72 * n))))


def _solve(make, cap):
    from krypy_amd import _hip, utils

    ctx = _hip.get_context()
    ctx.sync()
    t0 = time.perf_counter()
    try:
        sol = make()
        ok = True
    except utils.ConvergenceError as e:
        sol, ok = e.solver, False
    ctx.sync()
    return dict(seconds=time.perf_counter() - t0, iterations=len(sol.resnorms) - 1, converged=ok, last_resnorm=float(sol.resnorms[-1]))


def bench_solve(nx, ny, cap, tol=1e-8):
    from krypy_amd import linsys, utils

    A = cc.lap2d(nx, ny)
    n = A.shape[0]
    b = np.random.default_rng(1).standard_normal((n, 1))
    t0 = time.perf_counter()
    precs = [("plain", None), ("jacobi", sp.diags(1.0 / A.diagonal()).tocsr()),
             ("chebyshev4", utils.chebyshev_operator(A, degree=4)), ("chebyshev8", utils.chebyshev_operator(A, degree=8))]
    t_setup = time.perf_counter() - t0
    for name, M in precs:
        kw = dict(self_adjoint=True, positive_definite=True)
        if M is not None:
            kw["M"] = M
        applications = (M.degree - 1) if hasattr(M, "degree") else 0
        runs = (("cg", lambda: linsys.Cg(linsys.LinearSystem(A, b, **kw), tol=tol, maxiter=cap)),
                ("gmres100", lambda: linsys.RestartedGmres(linsys.LinearSystem(A, b, **kw), tol=tol, maxiter=100,
                                                           max_restarts=max(cap // 100 - 1, 0))))
        for solver, make in runs:
            r = _solve(make, cap)
            print(json.dumps(dict(what="solve", n=n, grid=[nx, ny], tol=tol, solver=solver, preconditioner=name,
                                  lmax=getattr(M, "lmax", None), operator_applications_per_iteration=1 + applications,
                                  setup_all_preconditioners_s=t_setup, **r)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,solve")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cap", type=int, default=20000)
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    what = args.what.split(",")
    if "kernels" in what:
        bench_kernels(ctx, "lap2d 1000 x 1000", cc.lap2d(1000, 1000), 8.0, args.reps)
        R = cc.random_spd(10 ** 6, 7, seed=0)
        bench_kernels(ctx, "random symmetric, ~7 per row", R, cc.gershgorin_lmax(R), args.reps)
        del R
        if args.big:
            bench_kernels(ctx, "lap2d 4000 x 2500", cc.lap2d(4000, 2500), 8.0, max(args.reps // 2, 5))
    if "solve" in what:
        if args.big:
            bench_solve(4000, 2500, args.cap)
        else:
            bench_solve(1000, 1000, args.cap)


if __name__ == "__main__":
    main()
