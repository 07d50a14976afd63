"""The rows of the chain-kernel dispatch (krypy_amd/csrc/chain_launch.hip: try_chain and its four stages, chain_blk2_step) as single
Arnoldi / Lanczos steps through ``kh_arnoldi_step_begin`` / ``_end`` and the complex entry: shared by
``tools/gen_chain_dispatch_golden.py`` (which records ``tests/golden/chain_dispatch.json``) and ``tests/test_gpu_chain_dispatch.py``
(which reproduces it).

A case is one upload and one step.  Sizes are the smallest that select the row on 256 compute units: the rows-per-lane class
``r2`` begins at ``n2 = r2_prev * 512 * 256 + 1`` double2 rows, i.e. ``n = 2 * n2`` doubles - a 2 x n2 grid of the five-point
Laplacian (``oracle.krylov_ref.laplace2d``: offsets -2, -1, 0, 1, 2) where the step has the operator in its prologue, no operator
at all (``A = None``: w is what the caller left in W) where it has not.  What is recorded per case: the deltas of the launch
counters and the SHA-256 of the returned H column (from ``start`` on) and of column k + 1 of the basis block(s).  Entries of the
H column before ``start`` (the Lanczos cases) are not written by the step - they hold whatever the slot held - and are therefore
not pinned.
"""
import ctypes
import functools
import hashlib

import numpy as np
import scipy.sparse as sp

from oracle import krylov_ref as ref

COUNTERS = ("n_chain_pf", "n_chain_xwin", "n_chain_onex", "n_chain_small", "n_chain_blk", "n_chain_blk2", "n_chain_long",
            "n_chain_xr", "n_lanczos_fused", "n_dia_mask")      # kh_ctx_get; n_chain, n_chain_lds, n_chain_fused: kh_ctx_counters


def _n2(r2_prev):
    return r2_prev * 512 * 256 + 1


# first vector length (doubles) of every rows-per-lane class on 256 compute units
N = {8: 2 * _n2(4), 16: 2 * _n2(8), 24: 2 * _n2(16), 32: 2 * _n2(24), 40: 2 * _n2(32), 48: 2 * _n2(40), 56: 2 * _n2(48)}
# complex vectors: one double2 row per entry
NZ = {16: _n2(8), 40: _n2(32)}
ONEX8 = 2 * (32 * 4 * 512 + 1)      # one XCD: 8 rows per lane from here on (4 rows up to 32 workgroups)


def case(name, n, k, op=None, start=0, sweeps=1, jacobi=False, cplx=False, unpadded=False, **switches):
    return dict(name=name, n=n, k=k, op=op, start=start, sweeps=sweeps, jacobi=jacobi, cplx=cplx, unpadded=unpadded,
                switches=switches)


def _lap(n):       # five-point Laplacian of n rows on a 2 x n / 2 grid
    assert n % 2 == 0
    return ("lap2d", 2, n // 2)


def _zlap(n):      # ... of n (odd) complex rows: the grid of n's smallest factor
    f = next(p for p in range(3, 100, 2) if n % p == 0)
    return ("zlap2d", f, n // f)


CASES = [
    # below 4,096 rows blocks are not padded to whole chunks: the MASKED ring (no preconditioner) and chain (Jacobi) kernels
    case("masked ring, 3000 rows", 3000, 3),
    case("masked chain (Jacobi), 3000 rows", 3000, 3, jacobi=True),
    case("masked chain (complex), 1500 rows", 1500, 3, cplx=True),
    # one XCD, >= 3 links: 4 rows per lane (ring; Jacobi: k_mgs_chain), 8 rows (ring excluded: Jacobi, and chain_small = 0: PF)
    case("one XCD, 4 rows, ring", 4096, 3),
    case("one XCD, 4 rows, ring, prologue", 4096, 3, op=_lap(4096)),
    case("one XCD, 4 rows, Jacobi", 4096, 3, jacobi=True),
    case("one XCD, 4 rows, Jacobi, prologue", 4096, 3, op=_lap(4096), jacobi=True),
    case("one XCD, 4 rows, PF (chain_small = 0)", 4096, 3, chain_small=0),
    case("one XCD, 4 rows, PF, prologue (chain_small = 0)", 4096, 3, op=_lap(4096), chain_small=0),
    case("one XCD, 8 rows, Jacobi", ONEX8, 3, jacobi=True),
    case("one XCD, 8 rows, Jacobi, prologue", ONEX8, 3, op=_lap(ONEX8), jacobi=True),
    case("one XCD, 8 rows, PF (chain_small = 0)", ONEX8, 3, chain_small=0),
    case("one XCD, 8 rows, PF, prologue (chain_small = 0)", ONEX8, 3, op=_lap(ONEX8), chain_small=0),
    case("one XCD, 4 rows, complex", 2048, 3, cplx=True),
    # k_mgs_chain_small spread over the chip: two links (no one-XCD grid), and the 8-row one-XCD shape the ring declines
    case("ring over the chip, 4 rows, two links", 4096, 1),
    case("ring over the chip, 4 rows (8 on one XCD declined)", ONEX8, 3),
    case("ring over the chip, 4 rows, prologue", ONEX8, 3, op=_lap(ONEX8)),
    case("ring over the chip, 8 rows", N[8], 3),
    case("ring over the chip, 8 rows, prologue", N[8], 3, op=_lap(N[8])),
    # the blocked kernel: k + 1 >= 8 links, on one XCD up to blk_onex_maxn rows, over the chip beyond
    case("blocked, one XCD", 4096, 8),
    case("blocked, one XCD, prologue", 4096, 8, op=_lap(4096)),
    case("blocked, over the chip", ONEX8, 8),
    case("blocked, over the chip, prologue", ONEX8, 8, op=_lap(ONEX8)),
    case("blk2, 8 rows", N[8], 8),
    # PF at 16 and 24 rows, LDS parking at 32 and 40 (x window on / off), long at 48 (on / off), 56
    case("PF, 16 rows", N[16], 1),
    case("PF, 16 rows, prologue", N[16], 1, op=_lap(N[16])),
    case("PF, 24 rows", N[24], 1),
    case("PF, 24 rows, prologue", N[24], 1, op=_lap(N[24])),
    case("LDS, 32 rows", N[32], 1),
    case("LDS, 32 rows, prologue, x window", N[32], 1, op=_lap(N[32])),
    case("LDS, 32 rows, prologue, chain_xwin = 0", N[32], 1, op=_lap(N[32]), chain_xwin=0),
    case("LDS, 32 rows, prologue, seven-point stencil", N[32] + 2, 1, op=("lap3d", 2, (N[32] + 2) // 4)),
    case("chain_lds = 0, 32 rows", N[32], 1, chain_lds=0),
    case("chain_lds = 0, 32 rows, prologue", N[32], 1, op=_lap(N[32]), chain_lds=0),
    case("LDS, 40 rows", N[40], 1),
    case("LDS, 40 rows, prologue, x window", N[40], 1, op=_lap(N[40])),
    case("LDS, 40 rows, prologue, chain_xwin = 0", N[40], 1, op=_lap(N[40]), chain_xwin=0),
    case("long, 48 rows", N[48], 1),
    case("long, 48 rows, prologue", N[48], 1, op=_lap(N[48])),
    case("48 rows, chain_long = 0", N[48], 1, chain_long=0),
    case("48 rows, chain_long = 0, prologue", N[48], 1, op=_lap(N[48]), chain_long=0),
    case("56 rows", N[56], 1),
    # Jacobi (B != V): the plain kernel
    case("Jacobi, 16 rows", N[16], 1, jacobi=True),
    case("Jacobi, 40 rows", N[40], 1, jacobi=True),
    case("Jacobi, 40 rows, prologue", N[40], 1, op=_lap(N[40]), jacobi=True),
    # complex
    case("complex, 16 rows", NZ[16], 1, cplx=True),
    case("complex, 16 rows, prologue", NZ[16], 1, op=_zlap(NZ[16]), cplx=True),
    case("complex, 40 rows", NZ[40], 1, cplx=True),
    case("complex, 40 rows, prologue", NZ[40], 1, op=_zlap(NZ[40]), cplx=True),
    # one link with the operator in the prologue: the Lanczos three-pass kernel
    case("Lanczos, 4 rows", 4096, 1, op=_lap(4096), start=1),
    case("Lanczos, 4 rows, Jacobi", 4096, 1, op=_lap(4096), start=1, jacobi=True),
    case("Lanczos, 16 rows", N[16], 1, op=_lap(N[16]), start=1),
    case("Lanczos, 16 rows, Jacobi", N[16], 1, op=_lap(N[16]), start=1, jacobi=True),
    case("Lanczos, 40 rows", N[40], 1, op=_lap(N[40]), start=1),
    case("Lanczos, 40 rows, Jacobi", N[40], 1, op=_lap(N[40]), start=1, jacobi=True),
    case("first step (k = 0), 40 rows, prologue", N[40], 0, op=_lap(N[40])),
    # blocks that are not padded to whole chunks (not what kh_vec_alloc hands out: the leading dimension is shortened by hand)
    case("unpadded block, 24 rows", N[24], 1, unpadded=True),
    case("unpadded block, 32 rows", N[32], 1, unpadded=True),
]
# (the operator of a case is built once and kept for its neighbours: cases of one size sit together above)


@functools.lru_cache(maxsize=2)
def _operator(op):
    kind, nx, ny = op
    A = ref.laplace3d(2, nx, ny) if kind == "lap3d" else ref.laplace2d(nx, ny)
    A.eliminate_zeros()      # (scipy's kron stores the zeros of a 2 x 2 identity block: a banded copy takes no stored zeros)
    if kind == "zlap2d":
        A = (A + sp.diags(1j * np.linspace(0.1, 0.5, A.shape[0]))).tocsr()
    return A


class _VecHead(ctypes.Structure):       # the head of kh_vec_s (kh_internal.h, which points back here): ctx, n, ncols, ld
    _fields_ = [("ctx", ctypes.c_void_p), ("n", ctypes.c_int64), ("ncols", ctypes.c_int64), ("ld", ctypes.c_int64)]


def _shorten_ld(block, by=32):
    """Shortens the leading dimension of a device block by `by` doubles (columns stay 256-byte aligned and inside the
    allocation): the block is then not padded to whole chunks of the chain kernels.  Returns the true value."""
    head = ctypes.cast(block.handle, ctypes.POINTER(_VecHead)).contents
    true_ld = head.ld
    assert head.n == block.n and head.ncols == block.ncols and true_ld - by >= block.n, "kh_vec_s layout"
    head.ld = true_ld - by
    assert block.ld == true_ld - by
    return true_ld


def _restore_ld(block, true_ld):
    ctypes.cast(block.handle, ctypes.POINTER(_VecHead)).contents.ld = true_ld


def _counts(ctx):
    c = ctx.counters()
    out = {"n_chain": c["chain"], "n_chain_lds": c["chain_lds"], "n_chain_fused": c["chain_fused"]}
    out.update((key, ctx.get(key)) for key in COUNTERS)
    return out


def run_case(ctx, c):
    """One step of case `c` on context `ctx`: {"counters": {name: delta}, "h": sha256, "v": sha256}."""
    n, k, start = c["n"], c["k"], c["start"]
    dt = np.complex128 if c["cplx"] else np.float64
    rng = np.random.default_rng(20261019)
    X = rng.standard_normal((n, k + 1))
    if c["cplx"]:
        X = X + 1j * rng.standard_normal((n, k + 1))
    X /= np.linalg.norm(X, axis=0)
    w = rng.standard_normal(n) + (1j * rng.standard_normal(n) if c["cplx"] else 0.0)
    dj = np.linspace(0.5, 1.5, n)
    old = {key: ctx.get(key) for key in c["switches"]}
    V = W = P = None
    true_ld = []
    try:
        for key, value in c["switches"].items():
            ctx.set(key, value)
        A = ctx.csr(_operator(c["op"])) if c["op"] is not None else None
        Md = ctx.diag(dj) if c["jacobi"] else None
        V, W = ctx.alloc(n, k + 2, dtype=dt), ctx.alloc(n, 2, dtype=dt)
        if c["unpadded"]:                    # (before anything is written: rows [n, ld) of every column stay zero)
            true_ld = [(b, _shorten_ld(b)) for b in (V, W)]
        if c["jacobi"]:                      # V = Md P
            P = ctx.alloc(n, k + 2, dtype=dt)
            P.upload(0, X)
            V.upload(0, dj[:, None] * X)
        else:
            V.upload(0, X)
        W.upload(0, w)
        before = _counts(ctx)
        ctx.arnoldi_step_begin(A, Md, V, P, W, 0, k, start, c["sweeps"], 0, 0.75 if start > 0 else 0.0, 0)
        h = ctx.arnoldi_step_end(0, k + 2, cplx=c["cplx"])
        after = _counts(ctx)
        vnext = V.download(k + 1, 1)
        pnext = P.download(k + 1, 1) if P is not None else None
    finally:
        for b, ld in true_ld:
            _restore_ld(b, ld)
        for key, value in old.items():
            ctx.set(key, value)
    hv = hashlib.sha256(np.ascontiguousarray(vnext).tobytes())
    if pnext is not None:
        hv.update(np.ascontiguousarray(pnext).tobytes())
    return {"counters": {key: int(after[key] - before[key]) for key in after},
            "h": hashlib.sha256(np.ascontiguousarray(h[start:]).tobytes()).hexdigest(), "v": hv.hexdigest()}
