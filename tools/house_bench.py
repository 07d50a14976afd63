#!/usr/bin/env python
"""Arnoldi(ortho='house') over 100 steps on the 2-D Laplacian at N = 10^4 ... 10^7: the one-launch step (k_house_chain)
against the per-reflector path (ctx.set("house_chain", 0): what every step ran before the kernel existed), with
ortho='mgs' for scale - all three in one process, alternating, three timed repetitions each after one warm-up run.

Per variant: steps/s (host clock around 100 advance() calls, ended by a device synchronise; the basis is allocated
outside the timed region), device calls per step (every call of the host layer that enqueues at least one launch or
copy: operator, dot / axpy panels, entry reads and writes, the step kernels) and host waits per step (calls that return
device data to the host).  A device call is NOT a launch - one call may enqueue several kernels or copies; only the
k_house_chain count is exact.  Kernel launches per step come from a kernel trace of a fused run (rocprofv3 --kernel-trace).

--c128: the same on complex data - the Laplacian minus the shift (0.5 + 0.75i) I, a complex start vector; the one-launch
step is k_zhouse_chain (counter n_zhouse_chain), the columns are the same.  --reps R: timed repetitions (default 3).
    python tools/house_bench.py [--c128] [--reps R] [nx ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 100
REPS = 3

# methods of the context / of a device block that enqueue work; the ones in WAITS hand device data back to the host
CTX_CALLS = ("apply", "dot_panel", "axpy_panel", "nrm2", "vdiv", "waxpby", "house_step", "zhouse_step", "arnoldi_step",
             "arnoldi_step_begin", "arnoldi_step_end")
VEC_CALLS = ("get", "set", "zero", "zero_range", "copy_from")
WAITS = ("dot_panel", "nrm2", "house_step", "zhouse_step", "arnoldi_step", "arnoldi_step_end", "get")


class Tally(object):
    def __init__(self, ctx, vec_cls):
        self.calls = self.waits = 0
        self._undo = []
        for owner, names in ((type(ctx), CTX_CALLS), (vec_cls, VEC_CALLS)):
            for name in names:
                fn = getattr(owner, name, None)
                if fn is None:          # (a context without the complex step)
                    continue
                setattr(owner, name, self._wrap(name, fn))
                self._undo.append((owner, name, fn))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.calls += 1
            self.waits += name in WAITS
            return fn(*a, **kw)
        return counted

    def close(self):
        for owner, name, fn in self._undo:
            setattr(owner, name, fn)


def run(ctx, utils, A, v, ortho, steps):
    ar = utils.Arnoldi(A, v, maxiter=steps, ortho=ortho)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        ar.advance()
    ctx.sync()
    return time.perf_counter() - t0


def counter_of(ctx, key):
    """A counter of the context, 0 where the library does not know it (a build without the complex step)."""
    try:
        return ctx.get(key)
    except Exception:
        return 0


def main(sizes, c128=False, reps=REPS):
    import numpy as np
    import scipy.sparse as sp
    import bench
    from krypy_amd import _hip, utils

    ctx = _hip.get_context()
    variants = (("house fused", "house", 1), ("house per-reflector", "house", 0), ("mgs", "mgs", 1))
    counter, kernel = ("n_zhouse_chain", "k_zhouse_chain") if c128 else ("n_house_chain", "k_house_chain")
    for nx in sizes:
        A = bench.laplace2d(nx, nx)
        N = A.shape[0]
        rng = np.random.default_rng(0)
        v = rng.standard_normal((N, 1))
        if c128:
            A = (A.astype(np.complex128) - (0.5 + 0.75j) * sp.identity(N, dtype=np.complex128, format="csr")).tocsr()
            v = v + 1j * rng.standard_normal((N, 1))
        best, counts = {}, {}
        for name, ortho, sw in variants:                 # warm-up (code objects, the operator's upload) + the call counts
            ctx.set("house_chain", sw)
            k0, w0 = counter_of(ctx, counter), ctx.get("n_tag_waits")
            tally = Tally(ctx, _hip.DeviceVectors)
            try:
                run(ctx, utils, A, v, ortho, STEPS)
            finally:
                tally.close()
            counts[name] = (tally.calls / STEPS, tally.waits / STEPS, (counter_of(ctx, counter) - k0) / STEPS,
                            (ctx.get("n_tag_waits") - w0) / STEPS)
        for _ in range(reps):                            # alternating: a drift of the machine hits all three alike
            for name, ortho, sw in variants:
                ctx.set("house_chain", sw)
                dt = run(ctx, utils, A, v, ortho, STEPS)
                best.setdefault(name, []).append(STEPS / dt)
        ctx.set("house_chain", 1)
        for name, _, _ in variants:
            r = sorted(best[name])
            c = counts[name]
            print("N = %8d  %s %-20s %9.1f steps/s (median of %d; %.1f ... %.1f)  device calls/step %6.1f  host waits/step %6.1f"
                  "  %s launches/step %.2f  completion-tag waits/step %.2f"
                  % (N, "c128" if c128 else "f64 ", name, r[len(r) // 2], reps, r[0], r[-1], c[0], c[1], kernel, c[2], c[3]),
                  flush=True)
        f, p = sorted(best["house fused"])[reps // 2], sorted(best["house per-reflector"])[reps // 2]
        print("N = %8d  fused / per-reflector = %.2f x" % (N, f / p), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    c128 = "--c128" in args
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else REPS
    sizes = [int(a) for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--reps")]
    main(sizes or [100, 316, 1000, 3162], c128=c128, reps=reps)
