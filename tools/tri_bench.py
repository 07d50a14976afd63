"""Measurements of the sparse triangular solves (krypy_amd/csrc/tri.hip) for KERNELS.md; not part of bench.py.

    python tools/tri_bench.py [--what rb,levels,gmres] [--big 1]

rb      the red-black Gauss-Seidel factor D + L of the five-point operator at N = 10^6 (and 10^7 with --big 1): time per solve
        and bytes/s against kh_apply of the SAME matrix in the same run (two wide levels; the solve moves about the SpMV's bytes).
levels  the natural ordering at N = 10^6 (1999 levels of 1 .. 1000 rows): time per level with tri_narrow_rows = 1024 (one narrow
        run), 0 (every level a launch) and values between.
gmres   GMRES(60) at N = 10^6 with Ml = ilu_operator(spilu(A)) on the device against the host-callable twin
        LinearOperator(dot=ilu.solve) - what a user could pass before -, median of 5 runs each.
Every line printed is one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_lower(nx, ny, redblack):
    """D + L of the five-point Laplacian on nx x ny in natural or red-black order, built from index arrays."""
    p = np.arange(nx * ny, dtype=np.int64)
    ix, iy = p // ny, p % ny
    if redblack:
        red = ((ix + iy) % 2) == 0
        new = np.empty(nx * ny, dtype=np.int64)
        new[red] = np.arange(int(red.sum()))
        new[~red] = int(red.sum()) + np.arange(int((~red).sum()))
    else:
        new = p
    rows, cols = [new], [new]
    for ok, q in ((ix > 0, p - ny), (ix < nx - 1, p + ny), (iy > 0, p - 1), (iy < ny - 1, p + 1)):
        r, c = new[ok], new[q[ok]]
        keep = c < r
        rows.append(r[keep])
        cols.append(c[keep])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 4.0, -1.0)
    T = sp.csr_matrix((vals, (rows, cols)), shape=(nx * ny, nx * ny))
    T.sort_indices()
    return T


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def bench_rb(ctx, nx, ny, reps):
    T = grid_lower(nx, ny, True)
    n = T.shape[0]
    t = ctx.tri(T, True, False)
    A = ctx.csr(T)
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y = ctx.alloc(n, 1)
    ms_tri = timed(ctx, lambda: ctx.tri_solve(t, X, 0, Y, 0, 1), reps)
    ms_spmv = timed(ctx, lambda: ctx.apply(A, X, 0, Y, 0, 1), reps)
    info = t.info()
    nbytes = 12 * (T.nnz - n) + n * (8 + 8 + 8 + 8)       # off-diagonal values and columns, diagonal, row id + length, b, x
    print(json.dumps(dict(what="rb", n=n, nnz=T.nnz, info=info, slots_per_nnz=info["slots"] / T.nnz, ms_tri=ms_tri, ms_spmv=ms_spmv,
                          ratio=ms_tri / ms_spmv, gbs_tri=nbytes / ms_tri * 1e-6, gbs_spmv=(12 * T.nnz + 20 * n) / ms_spmv * 1e-6)))


def bench_levels(ctx, nx, ny, reps):
    T = grid_lower(nx, ny, False)
    n = T.shape[0]
    X = ctx.upload(np.random.default_rng(0).standard_normal((n, 1)))
    Y = ctx.alloc(n, 1)
    for narrow in (1024, 512, 256, 128, 64, 0):
        ctx.set("tri_narrow_rows", narrow)
        t = ctx.tri(T, True, False)
        ctx.set("tri_narrow_rows", 1024)
        ms = timed(ctx, lambda: ctx.tri_solve(t, X, 0, Y, 0, 1), reps)
        info = t.info()
        print(json.dumps(dict(what="levels", n=n, narrow_rows=narrow, levels=info["levels"], wide=info["wide_launches"],
                              narrow=info["narrow_launches"], slots_per_nnz=info["slots"] / T.nnz, ms=ms,
                              us_per_level=1e3 * ms / info["levels"])))


def bench_gmres(nx, ny, runs):
    from krypy_amd import linsys, utils

    # convection-diffusion, five-point, natural order; the convection term stays inside the grid lines (an entry that couples the
    # end of one line to the start of the next chains the rows of U: 217,535 levels at this size and 34.3 s per GMRES(60) against 0.97 s with the host callable,
    # profiles/tri_bench_gmres_coupled_lines.log)
    A = (sp.kron(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx)), sp.identity(ny))
         + sp.kron(sp.identity(nx), sp.diags([-1.0, 2.0, -0.7], [-1, 0, 1], shape=(ny, ny)))).tocsr()
    n = A.shape[0]
    t0 = time.perf_counter()
    ilu = spla.spilu(A.tocsc(), drop_tol=1e-2, fill_factor=2, permc_spec="NATURAL", diag_pivot_thresh=0.0)
    t_fact = time.perf_counter() - t0
    b = np.random.default_rng(1).standard_normal((n, 1))
    t0 = time.perf_counter()
    dev = utils.ilu_operator(ilu)
    dev.dot(b)                       # analysis + upload happen here, once
    t_setup = time.perf_counter() - t0
    host = utils.LinearOperator((n, n), float, dot=lambda X: ilu.solve(X))
    out = {}
    for name, Ml in (("device", dev), ("host_callable", host)):
        ts = []
        for _ in range(runs):
            ls = linsys.LinearSystem(A, b, Ml=Ml)
            t0 = time.perf_counter()
            try:
                sol = linsys.Gmres(ls, tol=1e-30, maxiter=60)
            except utils.ConvergenceError as e:
                sol = e.solver
            ts.append(time.perf_counter() - t0)
        out[name] = dict(median_s=float(np.median(ts)), all_s=ts, last_resnorm=float(sol.resnorms[-1]), iterations=len(sol.resnorms) - 1)
    levels = [op._device_tri(utils._hip.get_context()).info() for op in (dev.args[0], dev.args[1])] if hasattr(dev, "args") else None
    print(json.dumps(dict(what="gmres", n=n, nnz_L=int(ilu.L.nnz), nnz_U=int(ilu.U.nnz), t_factorise_s=t_fact, t_device_setup_s=t_setup,
                          plans=levels, speedup=out["host_callable"]["median_s"] / out["device"]["median_s"], **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="rb,levels,gmres")
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    what = args.what.split(",")
    if "rb" in what:
        bench_rb(ctx, 1000, 1000, args.reps)
        if args.big:
            bench_rb(ctx, 4000, 2500, args.reps)
    if "levels" in what:
        bench_levels(ctx, 1000, 1000, max(args.reps // 4, 3))
    if "gmres" in what:
        bench_gmres(1000, 1000, 5)


if __name__ == "__main__":
    main()
