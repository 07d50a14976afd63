"""Measurements of BiCGStab (krypy_amd/csrc/bicgstab.hip) for KERNELS.md 4.27; not part of bench.py.

    python tools/bicgstab_bench.py [--grids 1000x1000,4000x2500] [--steps 200] [--warmup 20] [--reps 5]

Two variants of the same recurrence on convdiff(nx, ny, 0.5, 0.25), b = ones, alternating within one process:
  fused     linsys.Bicgstab on the fused path (one bicgstab_step call and one host synchronisation per iteration)
  composed  the recurrence built here from the calls the package had before the fused kernels: apply, waxpby, dot_panel
            (two-column dot_panel calls where two sums share an operand; three host synchronisations per iteration)
Each repetition is one solve of `warmup` iterations (discarded) and one of `steps` iterations, wall clock around the call with
the device drained before and after; the fused solve includes what the solver does around its loop (copies, the final explicit
residual), the composed one does not.  Before anything is timed the first eight residual norms of the two must agree to 1e-9.
Prints one JSON object per grid: iterations/s (median, min, max of the repetitions), the algorithmic bytes per iteration - the
vector passes counted in the kernels' comments, two for <rt, v>, and per operator application one read of x, one write of y and
the CSR arrays - and their share of 8 TB/s."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support.bicgstab_cases import convdiff      # noqa: E402  (the matrix of the tests)

PEAK = 8e12


def kernel_passes():
    """the 'N vector passes:' of the four kernels' comments in bicgstab.hip"""
    text = open(os.path.join(ROOT, "krypy_amd", "csrc", "bicgstab.hip")).read()
    found = [int(m) for m in re.findall(r"(\d+) vector passes:", text)]
    assert len(found) == 4, found
    return found


def fused_solve(ls, niter):
    from krypy_amd import linsys, utils
    try:
        sol = linsys.Bicgstab(ls, tol=1e-300, maxiter=niter)
    except utils.ConvergenceError as e:
        sol = e.solver
    assert sol.iter == niter, sol.iter
    return sol.resnorms[:niter]          # (the last entry is the explicit residual)


def composed_solve(ctx, Amat, b_dev, bnorm, niter):
    """the iteration of include/krylov_hip.h from apply / waxpby / dot_panel: the same expressions, hence the same bits
    from the same scalars"""
    n = b_dev.n
    RR = ctx.alloc(n, 2)                 # rt | r      (one dot_panel call gives <rt, r> and <r, r>)
    ST = ctx.alloc(n, 2)                 # s | t       (... and <s, t>, <t, t>)
    W = ctx.alloc(n, 4)                  # p | v | y | scratch
    RT, R, S, T, P, V, Y, X = 0, 1, 0, 1, 0, 1, 2, 3
    for blk, c in ((RR, RT), (RR, R), (W, P)):
        blk.copy_from(c, b_dev, 0, 1)
    rho, rr = (float(x) for x in ctx.dot_panel(RR, 0, 2, RR, R))
    res = [np.sqrt(rr) / bnorm]
    rho_prev = alpha = omega = 0.0
    for k in range(niter):
        if k > 0:
            beta = (rho / rho_prev) * (alpha / omega)
            ctx.waxpby(W, X, 1.0, W, P, -omega, W, V)
            ctx.waxpby(W, P, 1.0, RR, R, beta, W, X)
        ctx.apply(Amat, W, P, W, V)
        sigma = float(ctx.dot_panel(RR, RT, 1, W, V)[0])
        alpha = rho / sigma
        ctx.waxpby(ST, S, 1.0, RR, R, -alpha, W, V)
        ctx.apply(Amat, ST, S, ST, T)
        theta, phi = (float(x) for x in ctx.dot_panel(ST, 0, 2, ST, T))
        omega = theta / phi
        ctx.waxpby(W, Y, 1.0, W, Y, alpha, W, P)
        ctx.waxpby(W, Y, 1.0, W, Y, omega, ST, S)
        ctx.waxpby(RR, R, 1.0, ST, S, -omega, ST, T)
        rho_prev = rho
        rho, rr = (float(x) for x in ctx.dot_panel(RR, 0, 2, RR, R))
        res.append(np.sqrt(rr) / bnorm)
    return res


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def bench(ctx, nx, ny, steps, warmup, reps):
    from krypy_amd import linsys
    A = convdiff(nx, ny, 0.5, 0.25)
    n = A.shape[0]
    b = np.ones(n)
    ls = linsys.LinearSystem(A, b)
    Amat = ls.MlAMr._device_matrix(ctx, np.float64)
    b_dev = ctx.upload(b)
    bnorm = float(ls.MMlb_norm)
    variants = {"fused": lambda k: fused_solve(ls, k), "composed": lambda k: composed_solve(ctx, Amat, b_dev, bnorm, k)}
    first = {name: np.array(fn(9)[1:9]) for name, fn in variants.items()}
    diff = float(np.max(np.abs(first["fused"] - first["composed"]) / first["composed"]))
    assert diff <= 1e-9, "the two variants part company in the first eight iterations: %g" % diff
    its = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            fn(warmup)
            its[name].append(steps / timed(ctx, lambda: fn(steps)))
    passes = kernel_passes()
    vec = 8 * n * (sum(passes) + 2 + 2 * 2)
    mat = 2 * (12 * A.nnz + 4 * (n + 1))
    out = dict(what="bicgstab", grid=[nx, ny], n=n, nnz=int(A.nnz), diagonals=getattr(Amat, "diagonals", None), steps=steps, warmup=warmup, reps=reps,
               first8_max_rel_diff=diff, kernel_passes=passes, vector_bytes_per_iteration=vec, csr_bytes_per_iteration=mat)
    for name, v in its.items():
        med = float(np.median(v))
        out[name] = dict(iterations_per_s=med, min=float(min(v)), max=float(max(v)), all=[float(x) for x in v])
    f = out["fused"]["iterations_per_s"]
    out["fused_over_composed"] = f / out["composed"]["iterations_per_s"]
    out["separated"] = bool(out["fused"]["min"] > out["composed"]["max"])       # beats it by more than the spread of the repetitions
    out["share_of_peak_vectors"] = vec * f / PEAK
    out["share_of_peak_vectors_and_csr"] = (vec + mat) * f / PEAK
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="1000x1000,4000x2500")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    for g in args.grids.split(","):
        nx, ny = (int(x) for x in g.split("x"))
        bench(ctx, nx, ny, args.steps, args.warmup, args.reps)


if __name__ == "__main__":
    main()
