"""Measurements of the ILU(0) factorisation (krypy_amd/csrc/ilu0.hip) for KERNELS.md section 4.23; not part of bench.py.

    python tools/ilu0_bench.py [--what factor,gmres] [--big 1] [--out profiles/ilu0_bench.log]

factor  the five-point Laplacian at N = 10^6 (and 4000 x 2500 = 10^7 with --big 1), natural and multicolour order: the device
        time of the factorisation's launches (HIP events around them, "ilu0_device_us"), the wall time of the whole
        Context.ilu0 call (analysis, upload, launches, download) and of utils.ilu0 (plus colouring, permutation and the split
        into L and U), next to one kh_apply of the same matrix.
gmres   GMRES(60) - restarted, tol 1e-8, at most 50 cycles - on the N = 10^6 convection-diffusion operator of tools/tri_bench.py
        with five preconditioners as Ml: none; Chebyshev degree 4; ILU(0) natural; ILU(0) multicolour; the same multicolour
        factors applied by a host callable (two scipy spsolve_triangular and the permutations).  Iterations and seconds per
        solve, median of 5 (a host-callable solve that takes longer than --slow seconds is run once).
Every line printed (and written to --out) is one JSON object; the first carries the source stamp of the build."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_out = []


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    _out.append(line)


def source_stamp():
    """sha256 over the sources the library is built from, and the library's own."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "krypy_amd", "csrc")
    for fn in sorted(os.listdir(csrc)) + [os.path.join(ROOT, "include", "krylov_hip.h")]:
        path = fn if os.path.isabs(fn) else os.path.join(csrc, fn)
        if os.path.isfile(path) and path.endswith((".hip", ".h", "Makefile")):
            h.update(open(path, "rb").read())
    from krypy_amd import _hip
    lib = hashlib.sha256(open(_hip.library_path(), "rb").read()).hexdigest()
    return dict(sources_sha256=h.hexdigest()[:16], library_sha256=lib[:16])


def lap2d(nx, ny):
    A = (sp.kron(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx)), sp.identity(ny))
         + sp.kron(sp.identity(nx), sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(ny, ny)))).tocsr()
    A.sort_indices()
    return A


def bench_factor(ctx, nx, ny, reps):
    from krypy_amd import utils

    A = lap2d(nx, ny)
    n = A.shape[0]
    dA = ctx.csr(A)
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y = ctx.alloc(n, 1)
    ctx.apply(dA, X, 0, Y, 0, 1)
    ctx.sync()
    ctx.timer_start()
    for _ in range(20):
        ctx.apply(dA, X, 0, Y, 0, 1)
    ms_spmv = ctx.timer_stop() / 20
    for ordering in ("natural", "multicolor"):
        t0 = time.perf_counter()
        f = utils.ilu0(A, ordering)
        t_utils = time.perf_counter() - t0
        B = A[f.perm][:, f.perm].tocsr() if ordering == "multicolor" else A
        B.sort_indices()
        dev_us, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            lu, info = ctx.ilu0(B)
            wall.append(time.perf_counter() - t0)
            dev_us.append(ctx.get("ilu0_device_us"))
        emit(what="factor", nx=nx, ny=ny, n=n, nnz=A.nnz, ordering=ordering, info=info, colors=f.info["colors"],
             device_ms=float(np.median(dev_us)) / 1e3, device_ms_all=[u / 1e3 for u in dev_us], call_wall_s=float(np.median(wall)),
             utils_ilu0_wall_s=t_utils, spmv_ms=ms_spmv, device_over_spmv=float(np.median(dev_us)) / 1e3 / ms_spmv)


def bench_gmres(ctx, nx, ny, runs, slow):
    from krypy_amd import linsys, utils

    # the convection-diffusion operator of tools/tri_bench.py: the convection term stays inside the grid lines
    A = (sp.kron(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx)), sp.identity(ny))
         + sp.kron(sp.identity(nx), sp.diags([-1.0, 2.0, -0.7], [-1, 0, 1], shape=(ny, ny)))).tocsr()
    A.sort_indices()
    n = A.shape[0]
    b = np.random.default_rng(1).standard_normal((n, 1))
    setup = {}

    def timed_setup(name, make):
        t0 = time.perf_counter()
        op = make()
        if op is not None:
            op.dot(b)          # analysis + upload of the triangular operators happen here, once
        setup[name] = time.perf_counter() - t0
        return op

    f_mc = utils.ilu0(A, "multicolor")
    p, L, U = f_mc.perm, f_mc.L.tocsr(), f_mc.U.tocsr()

    def host_solve(X):
        Z = spla.spsolve_triangular(U, spla.spsolve_triangular(L, X[p], lower=True, unit_diagonal=True), lower=False)
        out = np.empty_like(Z)
        out[p] = Z
        return out

    precs = [("none", lambda: None), ("chebyshev_4", lambda: utils.chebyshev_operator(A, degree=4)),
             ("ilu0_natural", lambda: utils.ilu0_operator(A, "natural")), ("ilu0_multicolor", lambda: utils.ilu_operator(f_mc)),
             ("ilu0_multicolor_host_callable", lambda: utils.LinearOperator((n, n), float, dot=host_solve))]
    for name, make in precs:
        Ml = timed_setup(name, make)
        ts, its, ok = [], None, None
        for r in range(runs):
            ls = linsys.LinearSystem(A, b, **({} if Ml is None else {"Ml": Ml}))
            t0 = time.perf_counter()
            try:
                sol = linsys.RestartedGmres(ls, tol=1e-8, maxiter=60, max_restarts=49)
                ok = True
            except utils.ConvergenceError as e:
                sol, ok = e.solver, False
            ts.append(time.perf_counter() - t0)
            its = len(sol.resnorms) - 1
            if ts[-1] > slow:
                break
        plans = None
        if name.startswith("ilu0") and hasattr(Ml, "args"):
            tris, stack = [], [Ml]
            while stack:          # the product Pc * Uinv * Linv * Pr is nested
                o = stack.pop()
                stack += list(getattr(o, "args", []))
                if isinstance(o, utils.TriangularSolveOperator):
                    tris.append(o)
            plans = [dict(o._device_tri(ctx).info(), lower=o.lower) for o in tris]
        emit(what="gmres", n=n, prec=name, converged=ok, iterations=its, last_resnorm=float(sol.resnorms[-1]), median_s=float(np.median(ts)),
             all_s=ts, runs=len(ts), setup_s=setup[name], tri_plans=plans)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="factor,gmres")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow", type=float, default=20.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ilu0_bench.log"))
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    what = args.what.split(",")
    # the settings that shape the measurement (where the lines are written is not one of them)
    emit(what="stamp", compute_units=ctx.info()["compute_units"], measured=what, big=args.big, reps=args.reps, slow=args.slow,
         **source_stamp())
    try:
        if "factor" in what:
            bench_factor(ctx, 1000, 1000, args.reps)
            if args.big:
                bench_factor(ctx, 4000, 2500, args.reps)
        if "gmres" in what:
            bench_gmres(ctx, 1000, 1000, 5, args.slow)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()
