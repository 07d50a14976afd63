"""Measurements of IDR(s) (krypy_amd/csrc/idrs.hip) for KERNELS.md 4.28; not part of bench.py.

    python tools/idrs_bench.py [--grids 1000x1000,4000x2500] [--s 4] [--steps 200] [--warmup 20] [--reps 5]

Three variants of the same recurrence on convdiff(nx, ny, 0.5, 0.25), b = ones, alternating within one process:
  run       linsys.Idrs through idrs_run (s + 1 iterations per device call and host synchronisation)
  pieces    linsys.Idrs through idrs_dir / apply / idrs_orth and apply / idrs_omega (one synchronisation per iteration): the
            same solver on a context that hides idrs_run
  composed  the recurrence built here from apply / waxpby / dot_panel with the small scalars formed on the host by the
            reference's forward substitutions (two or three synchronisations per iteration)
Each repetition is one solve of `warmup` iterations (discarded) and one of `steps` iterations, wall clock around the call with
the device drained before and after; the solver's variants include what the solver does around its loop (allocations, the final
explicit residual; the shadow space is on the device already), the composed one does not.  Before anything is timed the
residual norms of the first cycle (and up to eight iterations) of run and pieces must be identical and the composed form's
must agree with them to 2e-9, the bound of the tests.  Prints one JSON object per grid: iterations/s
(median, min, max of the repetitions), the algorithmic bytes per iteration - the vector passes of a cycle counted as in
idrs.hip's header, and per operator application one read of x, one write of y and the CSR arrays - and their share of 8 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support import idrs_ref as ref                # noqa: E402  (the forward substitutions of the composed variant)
from tests.support.bicgstab_cases import convdiff      # noqa: E402  (the matrix of the tests)

PEAK = 8e12
L = ref.L


def cycle_passes(s):
    """vector passes of one cycle in the fused kernels and the block dots (idrs.hip's header)"""
    k_dir = sum(2 * (s - k) + 2 for k in range(s))
    k_orth = sum(7 if k == 0 else 2 * k + 8 for k in range(s))
    dots = s * (s + 1) + 2 + (s + 1)
    return dict(k_idr_dir=k_dir, k_idr_orth=k_orth, k_idr_omega=5, dots=dots, total=k_dir + k_orth + 5 + dots)


class WithoutRun(object):
    """the context with idrs_run hidden: linsys.Idrs takes the pieces"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        if name == "idrs_run":
            raise AttributeError(name)
        return getattr(self._ctx, name)


def solver_solve(ls, P, s, niter):
    from krypy_amd import linsys, utils
    try:
        sol = linsys.Idrs(ls, s=s, shadow=P, tol=1e-300, maxiter=niter)
    except utils.ConvergenceError as e:
        sol = e.solver
    assert sol.iter == niter, sol.iter
    return sol.resnorms[:niter]          # (the last entry is the explicit residual)


def composed_solve(ctx, Amat, b_dev, P, bnorm, s, niter):
    """the iteration of include/krylov_hip.h from apply / waxpby / dot_panel: the same expressions, the small scalars from
    the reference's forward substitutions on the host"""
    n = b_dev.n
    G, U = ctx.alloc(n, s), ctx.alloc(n, s)
    RT = ctx.alloc(n, 2)                 # r | t       (one dot_panel call gives <r, t> and <t, t>)
    W = ctx.alloc(n, 2)                  # y | v
    R, T, Y, V = 0, 1, 0, 1
    RT.copy_from(R, b_dev, 0, 1)
    sc = ref.new_scalars()
    sc[L["F"]: L["F"] + s] = ctx.dot_panel(P, 0, s, RT, R)
    sc[L["RR"]] = float(ctx.dot_panel(RT, R, 1, RT, R)[0])
    res = [np.sqrt(sc[L["RR"]]) / bnorm]
    for it in range(niter):
        k = it % (s + 1)
        if k < s:
            c, _ = ref.csolve(sc, k, s)
            ctx.waxpby(W, V, 1.0, RT, R, -c[k], G, k)
            for i in range(k + 1, s):
                ctx.waxpby(W, V, 1.0, W, V, -c[i], G, i)
            ctx.waxpby(U, k, float(sc[L["OM"]]), W, V, c[k], U, k)
            for i in range(k + 1, s):
                ctx.waxpby(U, k, 1.0, U, k, c[i], U, i)
            ctx.apply(Amat, U, k, RT, T)
            sc[L["H"]: L["H"] + s] = ctx.dot_panel(P, 0, s, RT, T)
            a, col, beta, fnew, _ = ref.asolve(sc, k, s)
            if k == 0:
                G.copy_from(k, RT, T, 1)
            for i in range(k):
                ctx.waxpby(G, k, 1.0, G if i else RT, k if i else T, -a[i], G, i)
                ctx.waxpby(U, k, 1.0, U, k, -a[i], U, i)
            for i in range(k, s):
                sc[L["M"] + i * ref.SM + k] = col[i - k]
            sc[L["F"] + k + 1: L["F"] + s] = fnew
            ctx.waxpby(RT, R, 1.0, RT, R, -beta, G, k)
            ctx.waxpby(W, Y, 1.0, W, Y, beta, U, k)
        else:
            ctx.apply(Amat, RT, R, RT, T)
            theta, phi = (float(x) for x in ctx.dot_panel(RT, 0, 2, RT, T))
            om, _ = ref.omega_scalars(theta, phi, sc[L["RR"]])
            sc[L["OM"]] = om
            ctx.waxpby(W, Y, 1.0, W, Y, om, RT, R)
            ctx.waxpby(RT, R, 1.0, RT, R, -om, RT, T)
            sc[L["F"]: L["F"] + s] = ctx.dot_panel(P, 0, s, RT, R)
        sc[L["RR"]] = float(ctx.dot_panel(RT, R, 1, RT, R)[0])
        res.append(np.sqrt(sc[L["RR"]]) / bnorm)
    return res


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def bench(ctx, nx, ny, s, steps, warmup, reps):
    from krypy_amd import linsys, utils
    A = convdiff(nx, ny, 0.5, 0.25)
    n = A.shape[0]
    b = np.ones(n)
    ls = linsys.LinearSystem(A, b)
    ls_pieces = linsys.LinearSystem(A, b)
    ls_pieces._ctx = WithoutRun(ctx)
    Amat = ls.MlAMr._device_matrix(ctx, np.float64)
    b_dev = ctx.upload(b)
    P = ctx.upload(utils.idrs_shadow(n, s, 0))
    bnorm = float(ls.MMlb_norm)
    variants = {"run": lambda k: solver_solve(ls, P, s, k), "pieces": lambda k: solver_solve(ls_pieces, P, s, k),
                "composed": lambda k: composed_solve(ctx, Amat, b_dev, P, bnorm, s, k)}
    m = max(s + 1, 8)
    first = {name: np.array(fn(m + 1)[1: m + 1]) for name, fn in variants.items()}
    assert np.array_equal(first["run"], first["pieces"]), "run and pieces do not compute the same bits"
    diff = float(np.max(np.abs(first["run"] - first["composed"]) / first["composed"]))
    assert diff <= 2e-9, "the variants part company in the first cycle: %g" % diff
    its = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            fn(warmup)
            its[name].append(steps / timed(ctx, lambda: fn(steps)))
    passes = cycle_passes(s)
    vec = 8.0 * n * (passes["total"] + 2 * (s + 1)) / (s + 1)
    mat = 12.0 * A.nnz + 4 * (n + 1)
    out = dict(what="idrs", s=s, grid=[nx, ny], n=n, nnz=int(A.nnz), steps=steps, warmup=warmup, reps=reps,
               first_max_rel_diff_composed=diff, cycle_passes=passes, vector_bytes_per_iteration=vec,
               csr_bytes_per_iteration=mat)
    for name, v in its.items():
        out[name] = dict(iterations_per_s=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=[float(x) for x in v])
    r = out["run"]["iterations_per_s"]
    out["run_over_composed"] = r / out["composed"]["iterations_per_s"]
    out["run_over_pieces"] = r / out["pieces"]["iterations_per_s"]
    out["run_separated_from_composed"] = bool(out["run"]["min"] > out["composed"]["max"])
    out["pieces_separated_from_composed"] = bool(out["pieces"]["min"] > out["composed"]["max"])
    out["run_separated_from_pieces"] = bool(out["run"]["min"] > out["pieces"]["max"])
    out["share_of_peak_vectors"] = vec * r / PEAK
    out["share_of_peak_vectors_and_csr"] = (vec + mat) * r / PEAK
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="1000x1000,4000x2500")
    ap.add_argument("--s", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    for g in args.grids.split(","):
        nx, ny = (int(x) for x in g.split("x"))
        bench(ctx, nx, ny, args.s, args.steps, args.warmup, args.reps)


if __name__ == "__main__":
    main()
