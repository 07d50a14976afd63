"""Measurements of the factorized sparse approximate inverse (krypy_amd/csrc/fsai.hip) for KERNELS.md section 4.26; not part of
bench.py.

    python tools/fsai_bench.py [--what build,apply,cg] [--big 1] [--out profiles/fsai_bench.log]

build   the five-point Laplacian at N = 10^6 (and 4000 x 2500 = 10^7 with --big 1), patterns tril(A) (q = 3) and tril(A^2) (q = 7):
        the device time of the one launch (HIP events around it, "fsai_device_us"; median of 5), the wall time of the whole
        Context.fsai call (validation, upload, launch, download) and of utils.fsai; in the same run k_spai on the pattern of A
        ("spai_device_us") and one kh_apply of A.
apply   one application of each form of utils.fsai_operator (factored: two kh_apply; matrix: one) next to one kh_apply of A.
cg      CG to 1e-8 on the N = 10^6 Laplacian: no preconditioner; spai(symmetric=True) on the patterns of A and A^2; FSAI in both
        forms on tril(A) and tril(A^2).  Iterations and seconds per solve, median of 5; the time to build each.
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


def lower(P):
    T = sp.tril(P).tocsr()
    T.sort_indices()
    return T


def _spmv_ms(ctx, M, X, Y):
    dM = ctx.csr(M)
    ctx.apply(dM, X, 0, Y, 0, 1)
    ctx.sync()
    ctx.timer_start()
    for _ in range(20):
        ctx.apply(dM, X, 0, Y, 0, 1)
    return ctx.timer_stop() / 20


def _op_ms(ctx, op, X, Y):
    op._apply_dev(X, 0, Y, 0, 1)
    ctx.sync()
    ctx.timer_start()
    for _ in range(20):
        op._apply_dev(X, 0, Y, 0, 1)
    return ctx.timer_stop() / 20


def bench_build(ctx, nx, ny, reps):
    from krypy_amd import utils

    A = lap2d(nx, ny)
    n = A.shape[0]
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y = ctx.alloc(n, 1)
    ms_a = _spmv_ms(ctx, A, X, Y)
    spai_us = []
    for _ in range(reps):
        ctx.spai(A, A)
        spai_us.append(ctx.get("spai_device_us"))
    for name in ("tril_A", "tril_A2"):
        given = None if name == "tril_A" else (A @ A).tocsr()
        P = lower(A if given is None else given)
        t0 = time.perf_counter()
        utils.fsai(A, given)
        t_utils = time.perf_counter() - t0
        dev_us, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, _, info = ctx.fsai(A, P)
            wall.append(time.perf_counter() - t0)
            dev_us.append(ctx.get("fsai_device_us"))
        emit(what="build", nx=nx, ny=ny, n=n, nnz=A.nnz, pattern=name, info=info, device_ms=float(np.median(dev_us)) / 1e3,
             device_ms_all=[u / 1e3 for u in dev_us], call_wall_s=float(np.median(wall)), utils_fsai_wall_s=t_utils, spmv_A_ms=ms_a,
             device_over_spmv_A=float(np.median(dev_us)) / 1e3 / ms_a, spai_pattern_A_device_ms=float(np.median(spai_us)) / 1e3)


def bench_apply(ctx, nx, ny):
    from krypy_amd import utils

    A = lap2d(nx, ny)
    n = A.shape[0]
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y = ctx.alloc(n, 1)
    ms_a = _spmv_ms(ctx, A, X, Y)
    for name in ("tril_A", "tril_A2"):
        given = None if name == "tril_A" else (A @ A).tocsr()
        fac = utils.fsai_operator(A, pattern=given, check=False)
        mat = utils.fsai_operator(A, pattern=given, form="matrix", check=False)
        emit(what="apply", n=n, pattern=name, nnz_A=A.nnz, nnz_G=fac.G.nnz, nnz_GhG=mat._A.nnz, spmv_A_ms=ms_a,
             factored_ms=_op_ms(ctx, fac, X, Y), matrix_ms=_op_ms(ctx, mat, X, Y))


def bench_cg(ctx, nx, ny, runs):
    from krypy_amd import linsys, utils

    A = lap2d(nx, ny)
    n = A.shape[0]
    b = np.random.default_rng(1).standard_normal((n, 1))
    A2 = (A @ A).tocsr()
    precs = [("none", lambda: None),
             ("spai_sym_A", lambda: utils.spai_operator(A, symmetric=True)),
             ("spai_sym_A2", lambda: utils.spai_operator(A, pattern=A2, symmetric=True)),
             ("fsai_matrix_tril_A", lambda: utils.fsai_operator(A, form="matrix")),
             ("fsai_factored_tril_A", lambda: utils.fsai_operator(A)),
             ("fsai_matrix_tril_A2", lambda: utils.fsai_operator(A, pattern=A2, form="matrix")),
             ("fsai_factored_tril_A2", lambda: utils.fsai_operator(A, pattern=A2))]
    for name, make in precs:
        try:
            t0 = time.perf_counter()
            op = make()
            if op is not None:
                op.dot(b)          # uploads happen here, once
            setup = time.perf_counter() - t0
            ts, its, ok = [], None, None
            for r in range(runs):
                ls = linsys.LinearSystem(A, b, self_adjoint=True, positive_definite=True, **({} if op is None else {"M": op}))
                t0 = time.perf_counter()
                try:
                    sol = linsys.Cg(ls, tol=1e-8, maxiter=6000)
                    ok = True
                except utils.ConvergenceError as e:
                    sol, ok = e.solver, False
                ts.append(time.perf_counter() - t0)
                its = len(sol.resnorms) - 1
            emit(what="cg", n=n, prec=name, converged=ok, iterations=its, last_resnorm=float(sol.resnorms[-1]),
                 median_s=float(np.median(ts)), all_s=ts, runs=len(ts), setup_s=setup)
        except (utils.ArgumentError, TypeError, ValueError) as e:          # a variant the solver refuses is reported (a device error ends the run)
            emit(what="cg", n=n, prec=name, error="%s: %s" % (type(e).__name__, e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="build,apply,cg")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsai_bench.log"))
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
        if "apply" in what:
            bench_apply(ctx, 1000, 1000)
        if "cg" in what:
            bench_cg(ctx, 1000, 1000, 5)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()
