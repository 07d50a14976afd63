"""Measurements of the persistent ILU(0) preconditioner (krypy_amd/csrc/ilu0p.hip) for KERNELS.md section 4.25; not part of
bench.py.

    python tools/ilu0p_bench.py [--what setup,apply,gmres] [--big 1] [--out profiles/ilu0p_bench.log]

setup   the five-point operator at 1000 x 1000 (and 4000 x 2500 with --big 1), natural and multicolour order: what new values of
        A cost - the wall time of Ilu0Preconditioner.update(A) next to "ilu0p_refactor_us" (HIP events around gather,
        factorisation and fill), against what the same job costs without the handle, utils.ilu0_operator(A, ordering) plus its
        first application, timed in the same process.  Median of --reps.  The one-time creation is reported too.
apply   one application: Ilu0Preconditioner._apply_dev against the composed ilu_operator, HIP events around 20 back-to-back
        applications, median of --reps; the launches per application from the counters.
gmres   GMRES(60) - restarted, tol 1e-8, at most 50 cycles - on the N = 10^6 convection-diffusion operator of tools/ilu0_bench.py
        under the multicolour ordering, with the persistent preconditioner and with ilu0_operator as Ml: iterations and seconds
        per solve, median of 5.
Every line printed (and written to --out) is one JSON object; the first carries the source stamp of the build."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.ilu0_bench import _out, emit, lap2d, source_stamp  # noqa: E402


def _counters(ctx, keys):
    return [ctx.get(k) for k in keys]


def bench_setup_and_apply(ctx, nx, ny, reps, what):
    from krypy_amd import precond, utils

    A = lap2d(nx, ny)
    n = A.shape[0]
    b = np.random.default_rng(0).standard_normal((n, 1))
    X = ctx.upload(b)
    Y = ctx.alloc(n, 1)
    for ordering in ("natural", "multicolor"):
        t0 = time.perf_counter()
        M = utils.Ilu0Preconditioner(A, ordering)
        ctx.sync()
        t_create = time.perf_counter() - t0
        if "setup" in what:
            upd, dev_us, old, call, canon = [], [], [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                M.update(A)
                ctx.sync()
                upd.append(time.perf_counter() - t0)
                dev_us.append(ctx.get("ilu0p_refactor_us"))
            # the C call alone (upload, launches, 4 bytes back) and the canonicalisation update() runs in front of it
            h = M._device_handle(ctx, M.dtype)
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.ilu0_refactor(h, M._A.data)
                call.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                precond._ilu0_canonical(A)
                canon.append(time.perf_counter() - t0)
            for _ in range(reps):
                t0 = time.perf_counter()
                op = utils.ilu0_operator(A, ordering)
                op._apply_dev(X, 0, Y, 0, 1)          # the triangular operators' analysis and upload happen here
                ctx.sync()
                old.append(time.perf_counter() - t0)
                del op
            emit(what="setup", nx=nx, ny=ny, n=n, nnz=A.nnz, ordering=ordering, info=M.info, create_wall_s=t_create,
                 update_wall_s=float(np.median(upd)), update_wall_s_all=upd, refactor_call_wall_s=float(np.median(call)),
                 canonicalise_wall_s=float(np.median(canon)), refactor_device_ms=float(np.median(dev_us)) / 1e3,
                 refactor_device_ms_all=[u / 1e3 for u in dev_us], h2d_bytes=ctx.get("ilu0p_h2d_bytes"),
                 d2h_bytes=ctx.get("ilu0p_d2h_bytes"), ilu0_operator_wall_s=float(np.median(old)), ilu0_operator_wall_s_all=old,
                 ratio=float(np.median(old)) / float(np.median(upd)))
        if "apply" in what:
            op = utils.ilu0_operator(A, ordering)
            res = {}
            for name, o, keys in (("persistent", M, ("n_ilu0p_wide", "n_ilu0p_narrow")), ("composed", op, ("n_tri_wide", "n_tri_narrow", "n_spmm"))):
                o._apply_dev(X, 0, Y, 0, 1)
                ctx.sync()
                c0 = _counters(ctx, keys)
                o._apply_dev(X, 0, Y, 0, 1)
                launches = dict(zip(keys, [a - b for a, b in zip(_counters(ctx, keys), c0)]))
                ms = []
                for _ in range(reps):
                    ctx.sync()
                    ctx.timer_start()
                    for _ in range(20):
                        o._apply_dev(X, 0, Y, 0, 1)
                    ms.append(ctx.timer_stop() / 20)
                res[name] = dict(ms=float(np.median(ms)), ms_all=ms, launches=launches)
            emit(what="apply", nx=nx, ny=ny, n=n, ordering=ordering, persistent=res["persistent"], composed=res["composed"],
                 ratio=res["composed"]["ms"] / res["persistent"]["ms"])
            del op
        del M


def bench_gmres(ctx, nx, ny, runs):
    from krypy_amd import linsys, utils

    A = (sp.kron(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx)), sp.identity(ny))
         + sp.kron(sp.identity(nx), sp.diags([-1.0, 2.0, -0.7], [-1, 0, 1], shape=(ny, ny)))).tocsr()
    A.sort_indices()
    n = A.shape[0]
    b = np.random.default_rng(1).standard_normal((n, 1))
    for name, make in (("ilu0_multicolor", lambda: utils.ilu0_operator(A, "multicolor")),
                       ("ilu0_multicolor_persistent", lambda: utils.Ilu0Preconditioner(A, "multicolor"))):
        t0 = time.perf_counter()
        Ml = make()
        Ml.dot(b)
        setup = time.perf_counter() - t0
        ts, its, ok = [], None, None
        for _ in range(runs):
            ls = linsys.LinearSystem(A, b, Ml=Ml)
            t0 = time.perf_counter()
            try:
                sol = linsys.RestartedGmres(ls, tol=1e-8, maxiter=60, max_restarts=49)
                ok = True
            except utils.ConvergenceError as e:
                sol, ok = e.solver, False
            ts.append(time.perf_counter() - t0)
            its = len(sol.resnorms) - 1
        emit(what="gmres", n=n, prec=name, converged=ok, iterations=its, last_resnorm=float(sol.resnorms[-1]), median_s=float(np.median(ts)),
             all_s=ts, runs=len(ts), setup_s=setup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="setup,apply,gmres")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ilu0p_bench.log"))
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    what = args.what.split(",")
    emit(what="stamp", compute_units=ctx.info()["compute_units"], measured=what, big=args.big, reps=args.reps, **source_stamp())
    try:
        if "setup" in what or "apply" in what:
            bench_setup_and_apply(ctx, 1000, 1000, args.reps, what)
            if args.big:
                bench_setup_and_apply(ctx, 4000, 2500, args.reps, what)
        if "gmres" in what:
            bench_gmres(ctx, 1000, 1000, 5)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(_out) + "\n")


if __name__ == "__main__":
    main()
