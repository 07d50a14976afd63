"""Measurements of the block-Jacobi preconditioner (krypy_amd/csrc/bjac.hip) for KERNELS.md 4.29; not part of bench.py.

    python tools/bjac_bench.py [--sizes 1000000,10000000] [--blocks 4,8,32] [--applies 50] [--reps 5] [--gmres 500x500x4]

Per size N and block size m: a block-diagonal matrix of random m x m blocks (standard normal plus 2 on the diagonal) on about N
rows, and its block-Jacobi preconditioner in two forms, alternating within one process:
  blocks    utils.BlockJacobiPreconditioner: the apply kernel k_bjac_apply on the inverses in their own layout
  matrix    MatrixLinearOperator of the same inverses as a CSR matrix: the library's CSR SpMV - the yardstick
Before anything is timed the two forms must give the same bits on one vector.  Each repetition is `applies` applications of one
form, wall clock around them with the device drained before and after, then the same for the other form; reported: microseconds
per application (median, min, max of the repetitions), the algorithmic bytes of an application of the blocks form - 8 W rows of
inverses, 16 rows of x and y - their share of 8 TB/s, and whether the two forms are separated by more than the spread.  The
build: wall clock of bjac_create (upload, launch, read-back of the breakdown word), the device time of its launch, and
numpy.linalg.inv over the same blocks on the host.  --gmres nx x ny x m: iterations/s of one GMRES(60) solve (three cycles) on
coupled(nx, ny, m) with each form as Ml.  Prints one JSON object per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.support.bjac_ref import coupled, group_width      # noqa: E402  (the test system)

PEAK = 8e12


def block_diagonal(n, m, seed):
    """(A as CSR, the blocks as an (nblk, m, m) array): n a multiple of m"""
    rng = np.random.default_rng(seed)
    nblk = n // m
    B = rng.standard_normal((nblk, m, m)) + 2.0 * np.eye(m)
    indptr = np.arange(0, n * m + 1, m, dtype=np.int64)
    indices = (np.arange(m, dtype=np.int32)[None, None, :] + (np.arange(nblk, dtype=np.int32) * m)[:, None, None]
               + np.zeros((1, m, 1), dtype=np.int32)).reshape(-1)
    A = sp.csr_matrix((B.reshape(-1), indices, indptr.astype(np.int32)), shape=(n, n))
    return A, B


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=[float(x) for x in v])


def bench_apply(ctx, N, m, applies, reps):
    from krypy_amd import utils
    n = (N // m) * m
    A, B = block_diagonal(n, m, 1)
    t0 = time.perf_counter()
    np.linalg.inv(B)
    host_inv_s = time.perf_counter() - t0
    del B
    t0 = time.perf_counter()
    P = utils.BlockJacobiPreconditioner(A, block_size=m)
    create_s = time.perf_counter() - t0
    build_us = ctx.get("bjac_device_us")
    info = P.info
    M = P.matrix()
    Pm = utils.MatrixLinearOperator(M)
    Md = Pm._device_matrix(ctx, np.float64)
    X = ctx.upload(np.random.default_rng(2).standard_normal(n))
    Y = ctx.alloc(n, 2)
    h = P._device_handle(ctx)
    forms = {"blocks": lambda: ctx.bjac_apply(h, X, 0, Y, 0, 1), "matrix": lambda: ctx.apply(Md, X, 0, Y, 1, 1)}
    forms["blocks"]()
    forms["matrix"]()
    y = Y.download()
    assert np.array_equal(y[:, 0].view(np.uint64), y[:, 1].view(np.uint64)), "the two forms do not compute the same bits"
    us = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            fn()
            us[name].append(1e6 * timed(ctx, lambda: [fn() for _ in range(applies)]) / applies)
    W = group_width(m)
    alg = 8.0 * W * n + 16.0 * n
    out = dict(what="bjac_apply", n=n, block=m, group_width=W, nblk=n // m, applies=applies, reps=reps, workgroups=info["workgroups"],
               device_bytes=info["device_bytes"], csr_bytes=12 * M.nnz + 4 * (n + 1), csr_diagonals=Md.diagonals,
               algorithmic_bytes=alg, create_wall_s=create_s, build_device_us=build_us, host_numpy_inv_s=host_inv_s)
    for name, v in us.items():
        out[name + "_us"] = stats(v)
    b, c = out["blocks_us"], out["matrix_us"]
    out["matrix_over_blocks"] = c["median"] / b["median"]
    out["blocks_separated_from_matrix"] = bool(b["max"] < c["min"])
    out["share_of_peak_blocks"] = alg / (b["median"] * 1e-6) / PEAK
    out["share_of_peak_matrix_csr_bytes"] = (out["csr_bytes"] + 16.0 * n) / (c["median"] * 1e-6) / PEAK
    print(json.dumps(out), flush=True)


def bench_gmres(ctx, nx, ny, m, reps):
    from krypy_amd import linsys, utils
    A = coupled(nx, ny, m, seed=2)
    n = A.shape[0]
    b = np.ones((n, 1))
    forms = {form: utils.block_jacobi_operator(A, block_size=m, form=form) for form in ("blocks", "matrix")}

    def solve(form):
        ls = linsys.LinearSystem(A, b, Ml=forms[form])
        try:
            sol = linsys.RestartedGmres(ls, tol=1e-300, maxiter=60, max_restarts=2)
        except utils.ConvergenceError as e:
            sol = e.solver
        return len(sol.resnorms) - 1

    its = {form: [] for form in forms}
    for _ in range(reps):
        for form in forms:
            count = [0]
            t = timed(ctx, lambda: count.__setitem__(0, solve(form)))
            its[form].append(count[0] / t)
    out = dict(what="bjac_gmres60", grid=[nx, ny, m], n=n, nnz=int(A.nnz), reps=reps)
    for form, v in its.items():
        out[form + "_iterations_per_s"] = stats(v)
    out["blocks_over_matrix"] = out["blocks_iterations_per_s"]["median"] / out["matrix_iterations_per_s"]["median"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--blocks", default="4,8,32")
    ap.add_argument("--applies", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gmres", default="500x500x4")
    args = ap.parse_args()
    from krypy_amd import _hip
    ctx = _hip.get_context()
    for N in (int(x) for x in args.sizes.split(",") if x):
        for m in (int(x) for x in args.blocks.split(",") if x):
            bench_apply(ctx, N, m, args.applies, args.reps)
    if args.gmres:
        nx, ny, m = (int(x) for x in args.gmres.split("x"))
        bench_gmres(ctx, nx, ny, m, args.reps)


if __name__ == "__main__":
    main()
