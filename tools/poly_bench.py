"""Measurements of the GMRES polynomial preconditioner (krypy_amd/csrc/poly.hip) for KERNELS.md; not part of bench.py.

    python tools/poly_bench.py [--what kernels,solve] [--big 1] [--reps 20] [--cap 20000]

kernels  time per step of ``y = p(A) x`` with an all-LIN table (real roots) on the five-point Laplacian (mask form) at N = 10^6
         (and 10^7 with --big 1): the fused epilogue against the composed path (kh_apply + k_poly_update), and beside them the
         fused Chebyshev step of kh_cheb_apply on the same matrix, all alternating within one process, device events around
         `reps` back-to-back applications after a warm-up, 5 rounds.  A step's time is the difference between the applications
         with 8 and with 4 steps, divided by 4 (what a further step costs, without the launch that writes the records).
solve    time to tol 1e-8 - wall clock around the solver call, the device drained - of restarted GMRES(100) on the 1000 x 1000
         Laplacian (and 4000 x 2500 with --big 1), b = ones: plain and with Mr = gmres_polynomial_operator at degree 8 and 16,
         with the iteration counts and the number of operator applications.  --cap bounds the iterations of one run; a run
         that stops there is reported with converged = false.
Every line printed is one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support import cheb_cases as cc      # noqa: E402  (the matrices of the tests)


def timed(ctx, fn, reps):
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def bench_kernels(ctx, name, A, reps, rounds=5):
    from krypy_amd.utils import chebyshev_coefficients, gmres_polynomial_steps

    n = A.shape[0]
    dm = ctx.csr(A)
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y, S = ctx.alloc(n, 1), ctx.alloc(n, 3)
    # real roots inside the spectrum's hull (0, 8): the numbers do not matter to the time
    tabs = {k: gmres_polynomial_steps(np.linspace(1.0, 7.0, k + 1)) for k in (4, 8)}
    coefs = {k: chebyshev_coefficients(8.0 / 30.0, 8.0, k + 1) for k in (4, 8)}

    def poly(k, fused):
        def run():
            ctx.set("poly_fused", fused)
            ctx.poly_apply(dm, tabs[k], X, 0, Y, 0, 1, S)
        return run

    def cheb(k):
        def run():
            ctx.cheb_apply(dm, None, coefs[k], X, 0, Y, 0, 1, S)
        return run

    def spmv(k):
        def run():
            for j in range(k):
                ctx.apply(dm, S if j % 2 else X, 1 if j % 2 else 0, S, 2 if j % 2 else 1, 1)
        return run

    variants = [("%s%d" % (what, k), make(k)) for k in (4, 8) for what, make in (
        ("poly_fused", lambda k: poly(k, 1)), ("poly_composed", lambda k: poly(k, 0)), ("cheb_fused", cheb), ("spmv_only", spmv))]
    for _, fn in variants:
        fn()
    ms = {k: [] for k, _ in variants}
    for _ in range(rounds):
        for k, fn in variants:
            ms[k].append(timed(ctx, fn, reps))
    ctx.set("poly_fused", 1)
    step = {what: [1e3 * (b - a) / 4 for a, b in zip(ms[what + "4"], ms[what + "8"])]
            for what in ("poly_fused", "poly_composed", "cheb_fused", "spmv_only")}
    print(json.dumps(dict(what="kernels", operator=name, n=n, nnz=int(A.nnz), diagonals=dm.diagonals,
                          us_per_step_median={k: float(np.median(v)) for k, v in step.items()}, us_per_step_rounds=step,
                          ms_per_application={k: float(np.median(v)) for k, v in ms.items()},
                          vector_bytes_model=dict(poly_fused_lin=32 * n, poly_composed_lin=56 * n, cheb_fused=40 * n))), flush=True)


def _solve(make):
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
    b = np.ones((n, 1))
    for degree in (0, 8, 16):
        t0 = time.perf_counter()
        Mr = utils.gmres_polynomial_operator(A, degree=degree) if degree else None
        t_setup = time.perf_counter() - t0
        kw = dict(Mr=Mr) if degree else {}
        r = _solve(lambda: linsys.RestartedGmres(linsys.LinearSystem(A, b, **kw), tol=tol, maxiter=100,
                                                 max_restarts=max(cap // 100 - 1, 0)))
        per_it = 1 + (Mr.steps.shape[0] if degree > 1 else 0)
        print(json.dumps(dict(what="solve", n=n, grid=[nx, ny], tol=tol, solver="gmres100", degree=degree, setup_s=t_setup,
                              log10_pof_max=Mr.info["log10_pof_max"] if degree else None,
                              operator_applications_per_iteration=per_it,
                              operator_applications=per_it * r["iterations"] + degree, **r)), flush=True)


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
        bench_kernels(ctx, "lap2d 1000 x 1000", cc.lap2d(1000, 1000), args.reps)
        if args.big:
            bench_kernels(ctx, "lap2d 4000 x 2500", cc.lap2d(4000, 2500), max(args.reps // 2, 5))
    if "solve" in what:
        bench_solve(1000, 1000, args.cap)
        if args.big:
            bench_solve(4000, 2500, args.cap)


if __name__ == "__main__":
    main()
