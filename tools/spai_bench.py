"""Measurements of the sparse approximate inverse (krypy_amd/csrc/spai.hip) for KERNELS.md section 4.24; not part of bench.py.

    python tools/spai_bench.py [--what build,gmres] [--big 1] [--out profiles/spai_bench.log]

build   the five-point Laplacian at N = 10^6 (and 4000 x 2500 = 10^7 with --big 1), pattern of A (q = 5) and of A^2 (q = 13): the
        device time of the one launch (HIP events around it, "spai_device_us"; median of 5), the wall time of the whole
        Context.spai call (validation, upload, launch, download) and of utils.spai, next to one kh_apply of A and one of M.
gmres   GMRES(60) - restarted, tol 1e-8, at most 50 cycles - on the N = 10^6 convection-diffusion operator of tools/ilu0_bench.py:
        no preconditioner; Chebyshev degree 4 and multicolour ILU(0) as Ml; SPAI(A) and SPAI(A^2) as Ml; the same two, symmetrised,
        as the inner-product preconditioner M.  Iterations and seconds per solve, median of 5; the time to build each.
Every line printed (and written to --out) is one JSON object; the first carries the source stamp of the build."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

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


def _spmv_ms(ctx, M, X, Y):
    dM = ctx.csr(M)
    ctx.apply(dM, X, 0, Y, 0, 1)
    ctx.sync()
    ctx.timer_start()
    for _ in range(20):
        ctx.apply(dM, X, 0, Y, 0, 1)
    return ctx.timer_stop() / 20


def bench_build(ctx, nx, ny, reps):
    from krypy_amd import utils

    A = lap2d(nx, ny)
    n = A.shape[0]
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y = ctx.alloc(n, 1)
    ms_a = _spmv_ms(ctx, A, X, Y)
    for name in ("A", "A2"):
        P = A if name == "A" else (A @ A).tocsr()
        P.sort_indices()
        t0 = time.perf_counter()
        M = utils.spai(A, None if name == "A" else P)
        t_utils = time.perf_counter() - t0
        dev_us, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, info = ctx.spai(A, P)
            wall.append(time.perf_counter() - t0)
            dev_us.append(ctx.get("spai_device_us"))
        ms_m = _spmv_ms(ctx, M, X, Y)
        emit(what="build", nx=nx, ny=ny, n=n, nnz=A.nnz, pattern=name, info=info, device_ms=float(np.median(dev_us)) / 1e3,
             device_ms_all=[u / 1e3 for u in dev_us], call_wall_s=float(np.median(wall)), utils_spai_wall_s=t_utils, spmv_A_ms=ms_a,
             spmv_M_ms=ms_m, device_over_spmv_A=float(np.median(dev_us)) / 1e3 / ms_a)


def bench_gmres(ctx, nx, ny, runs):
    from krypy_amd import linsys, utils

    # the convection-diffusion operator of tools/ilu0_bench.py: the convection term stays inside the grid lines
    A = (sp.kron(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx)), sp.identity(ny))
         + sp.kron(sp.identity(nx), sp.diags([-1.0, 2.0, -0.7], [-1, 0, 1], shape=(ny, ny)))).tocsr()
    A.sort_indices()
    n = A.shape[0]
    b = np.random.default_rng(1).standard_normal((n, 1))
    A2 = (A @ A).tocsr()
    precs = [("none", None, lambda: None), ("chebyshev_4", "Ml", lambda: utils.chebyshev_operator(A, degree=4)),
             ("ilu0_multicolor", "Ml", lambda: utils.ilu0_operator(A, "multicolor")),
             ("spai_A_Ml", "Ml", lambda: utils.spai_operator(A)), ("spai_A2_Ml", "Ml", lambda: utils.spai_operator(A, pattern=A2)),
             ("spai_A_M", "M", lambda: utils.spai_operator(A, symmetric=True)),
             ("spai_A2_M", "M", lambda: utils.spai_operator(A, pattern=A2, symmetric=True))]
    for name, key, make in precs:
        try:
            _one_gmres(linsys, utils, A, b, n, name, key, make, runs)
        except (utils.ArgumentError, TypeError, ValueError) as e:          # a variant the solver refuses is reported (a device error ends the run)
            emit(what="gmres", n=n, prec=name, hook=key, error="%s: %s" % (type(e).__name__, e))


def _one_gmres(linsys, utils, A, b, n, name, key, make, runs):
    t0 = time.perf_counter()
    op = make()
    if op is not None:
        op.dot(b)          # uploads and analyses happen here, once
    setup = time.perf_counter() - t0
    ts, its, ok = [], None, None
    for r in range(runs):
        ls = linsys.LinearSystem(A, b, **({} if op is None else {key: op}))
        t0 = time.perf_counter()
        try:
            sol = linsys.RestartedGmres(ls, tol=1e-8, maxiter=60, max_restarts=49)
            ok = True
        except utils.ConvergenceError as e:
            sol, ok = e.solver, False
        ts.append(time.perf_counter() - t0)
        its = len(sol.resnorms) - 1
    emit(what="gmres", n=n, prec=name, hook=key, converged=ok, iterations=its, last_resnorm=float(sol.resnorms[-1]),
         median_s=float(np.median(ts)), all_s=ts, runs=len(ts), setup_s=setup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="build,gmres")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spai_bench.log"))
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    what = args.what.split(",")
    # the settings that shape the measurement (where the lines are written is not one of them)
    emit(what="stamp", compute_units=ctx.info()["compute_units"], measured=what, big=args.big, reps=args.reps, **source_stamp())
    try:
        if "build" in what:
            bench_build(ctx, 1000, 1000, args.reps)
            if args.big:
                bench_build(ctx, 4000, 2500, args.reps)
        if "gmres" in what:
            bench_gmres(ctx, 1000, 1000, 5)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()
