"""Two storage contracts carry every fast kernel, and this file holds them on the device.

1. "Every column is written before it is read."  A Krylov basis is allocated with ``zero=False`` and the block pool hands a
   parked block out as it is, so whatever a kernel reads beyond the columns written so far - a look-ahead load, a prefetch of
   the column ring, the lanes of an unmasked kernel behind the vector's end - may be NaN.  Every case runs twice on fresh
   contexts, on zero-filled blocks and on blocks whose rows ``[0, n)`` are NaN in EVERY column (one more column allocated
   than the sequence writes), and the results must have the same bits.
2. "The padding is zero and stays zero."  Rows ``[n, ld)`` and the slack behind the last column are what lets the unmasked
   instantiations run without a predicate; ``DeviceVectors.padding_nonzero()`` (kh_vec_padding_nonzero) must be 0 after every
   sequence, exact breakdowns (a division by h = 0) included.

The clean run of every case is also compared with ``tests.support.poison.arnoldi_longdouble`` - extended precision, plain
NumPy, no code shared with the library or the fp64 oracle - at the bars the family's own test already holds it to against
another kernel or the oracle: 1e-12 ||H_ref|| and 1e-11 sqrt(m) for the five-step cases, 1e-11 ||H_ref|| and 1e-10 for the
12 - 14-step ring cases, 1e-10 for the blocked kernels.  For every real operator used here (tridiagonal with a varying
diagonal; the 5-point Laplacian as it is / with one entry one ulp off / with a sixth diagonal of size 0.01; with and without
the Jacobi diagonal linspace(0.5, 1.5); as a Lanczos run) the longdouble reference and ``oracle.krylov_ref.arnoldi_step`` were
compared on the CPU at reduced sizes of the same construction (n = 3,000 ... 60,000, the same step counts and sweeps): the
five- to seven-step runs agree to 1e-15 ||H|| and 5e-15 in the basis, the 12- and 14-step runs to 1.3e-14 ||H|| and 6e-14 in
the basis - a hundredth of their bars or less.  The oracle is real; for the complex operators (the same ones plus an imaginary
diagonal) tests/test_host_logic.py checks the Arnoldi relation and orthonormality of the reference in extended precision.

Which kernel took a step is stated through ``expect_kernel`` with the counters the families' own tests use: with a family
switched off on purpose every numeric assertion still runs on whatever kernel took the step."""
import functools
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as ref
from tests.support import poison as po
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

_COUNTERS = ("n_chain_small", "n_chain_onex", "n_chain_blk", "n_chain_blk2", "n_chain_long", "n_lanczos_fused", "n_dia_mask",
             "n_minres_rides")


def _counters(ctx):
    d = dict(ctx.counters())
    for key in _COUNTERS:
        d[key] = ctx.get(key)
    return d


def _nrm(x):
    return float(np.sqrt(np.sum(np.abs(x) ** 2)))


@functools.lru_cache(maxsize=2)
def _operator(kind, a, b=0):
    """Built once per size (consecutive cases share it)."""
    if kind in ("tri", "ztri"):              # the operator of test_mgs_chain_every_register_shape
        A = sp.diags([np.full(a - 1, -1.0), np.linspace(2.0, 3.0, a), np.full(a - 1, -1.0)], [-1, 0, 1]).tocsr()
        return (A + sp.diags(1j * np.linspace(0.1, 0.5, a))).tocsr() if kind == "ztri" else A
    A = ref.laplace2d(a, b)
    n = A.shape[0]
    if kind == "lap2d":                      # constant coefficients: the mask form of the banded copy
        return A
    if kind == "lap2d_value":                # one entry one ulp off: the value form (tests/test_gpu_dia_mask.py)
        A.data[A.nnz // 3] = np.nextafter(A.data[A.nnz // 3], 0.0)
        return A
    if kind == "lap2d_6":                    # six diagonals: no banded copy, the SpMV is a launch of its own
        return (A + sp.diags(np.random.default_rng(2).standard_normal(n - 37) * 0.01, 37, shape=(n, n))).tocsr()
    if kind == "zlap2d":
        return (A + 0.3j * sp.diags(np.random.default_rng(6).standard_normal(n))).tocsr()
    raise ValueError(kind)


def _sequence(ctx, c, A, v, dj, poisoned, blocks=None):
    """m Arnoldi / Lanczos steps of case `c` through kh_arnoldi_step on context `ctx`; with `poisoned`, every column of V, P
    and W is NaN before column 0 is uploaded.  `blocks`: run on these (V, P, W) as they are instead of new ones."""
    n, m = A.shape[0], c["m"]
    cplx, jac, lanczos = c.get("cplx", False), c.get("jacobi", False), c.get("lanczos", False)
    dt = complex if cplx else float
    wcol, sweeps, gs_mode = c.get("wcol", 0), c["sweeps"], c.get("gs_mode", 0)
    Ad = ctx.csr(A)
    Md = ctx.diag(dj, dtype=dt) if jac else None
    if blocks is None:
        V, W = ctx.alloc(n, m + 2, dtype=dt), ctx.alloc(n, 2, dtype=dt)
        P = ctx.alloc(n, m + 2, dtype=dt) if jac else None
    else:
        V, P, W = blocks
    if poisoned:
        for blk in (V, P, W):
            if blk is not None:
                po.poison(blk)
    if jac:
        nrm = np.sqrt(np.vdot(v, dj * v).real)
        P.upload(0, v / nrm)
        V.upload(0, dj * v / nrm)
    else:
        V.upload(0, v / np.linalg.norm(v))
    rides = c.get("rides", False)
    if rides:            # MINRES recurrences riding along in the Lanczos launch, as Minres defers them
        rng = np.random.default_rng(11)
        Wm, yk = ctx.upload(rng.standard_normal((n, 2))), ctx.upload(rng.standard_normal((n, 1)))
    H = np.zeros((m + 1, m), dtype=dt)
    for k in range(m):
        start = k if lanczos else 0
        hk = float(H[k, k - 1].real) if (lanczos and k > 0) else 0.0
        if rides and k >= 2:
            ctx.minres_update(V, k - 2, Wm, k & 1, 0.3, -0.2, 1.7, 0.4, yk, 0, defer=True)
        if c.get("external_w", False):       # the caller supplies w (A == NULL): only W's other column stays poisoned
            ctx.apply(Ad, V, k, W, wcol)
        hcol = ctx.arnoldi_step(None if c.get("external_w", False) else Ad, Md, V, P, W, wcol, k, start, sweeps[k], gs_mode, hk)
        H[start: k + 2, k] = hcol[start: k + 2]
        if lanczos and k > 0:
            H[k - 1, k] = H[k, k - 1]
    out = dict(H=H, V=V.download(0, m + 1), blocks=(V, P, W))
    if jac:
        out["P"] = P.download(0, m + 1)
    if rides:
        ctx.minres_flush()
        out["Wm"], out["yk"] = Wm.download(), yk.download()
    out["pad"] = [blk.padding_nonzero() for blk in (V, P, W) if blk is not None]
    return out


def _start_vector(c, n):
    rng = np.random.default_rng(c.get("seed", 3))
    v = rng.standard_normal(n)
    if c.get("cplx", False):
        v = v + 1j * rng.standard_normal(n)
    return v


def _run_case(c):
    """The three assertions of a family case; returns the counter differences of the two runs."""
    from krypy_amd import _hip

    A = _operator(*c["op"])
    n, m = A.shape[0], c["m"]
    v = _start_vector(c, n)
    dj = np.linspace(0.5, 1.5, n) if c.get("jacobi", False) else None
    res = {}
    for poisoned in (False, True):
        ctx = _hip.Context(0)
        try:
            for key, val in c.get("set", {}).items():
                ctx.set(key, val)
            c0 = _counters(ctx)
            res[poisoned] = _sequence(ctx, c, A, v, dj, poisoned)
            c1 = _counters(ctx)
            res[poisoned]["used"] = {k: c1[k] - c0[k] for k in c1}
            del res[poisoned]["blocks"]
        finally:
            ctx.close()
    clean, bad = res[False], res[True]
    print("KERNELS %s: %r" % (c["id"], clean["used"]))
    # 1. nothing unwritten was read: the same bits on poisoned blocks
    for key in ("H", "V", "P", "Wm", "yk"):
        if key in clean:
            po.bits_equal(bad[key], clean[key], "%s of the poisoned run against the clean one" % key)
    # 3. the padding is still zero
    assert bad["pad"] == [0] * len(bad["pad"]), "non-zero padding words of V, (P,) W after the poisoned run: %r" % (bad["pad"],)
    assert clean["pad"] == [0] * len(clean["pad"]), "non-zero padding words of V, (P,) W after the clean run: %r" % (clean["pad"],)
    # 2. the clean run against the extended-precision reference
    Href, Vref, Pref = po.arnoldi_longdouble(A, v, m, c["sweeps"], M_diag=dj, lanczos=c.get("lanczos", False))
    hbar, vbar = c["bars"]
    herr, href = _nrm(clean["H"] - Href), _nrm(Href)
    verr = _nrm(clean["V"] - Vref)
    perr = _nrm(clean["P"] - Pref) if "P" in clean else 0.0
    del Vref, Pref
    print("FIGURES %s: |H - H_ref| / |H_ref| = %.3e (bar %.0e), |V - V_ref| = %.3e, |P - P_ref| = %.3e (bar %.3e)"
          % (c["id"], herr / href, hbar, verr, perr, vbar))
    assert herr <= hbar * href, (herr / href, hbar)
    assert verr <= vbar, (verr, vbar)
    assert perr <= vbar, (perr, vbar)
    return clean["used"], bad["used"]


def _sw(m, at=(), every=1):
    """sweeps per step: `every`, and 2 at the steps `at`"""
    return tuple(2 if k in at else every for k in range(m))


_BAR5 = lambda m: (1e-12, 1e-11 * np.sqrt(m))      # the bars of test_mgs_chain_every_register_shape
_BAR_RING = (1e-11, 1e-10)                          # test_column_ring_kernel_for_short_vectors
_BAR_BLK = (1e-10, 1e-10)                           # tests/test_gpu_blocked.py, tests/test_gpu_blk2.py


# ---- masked chain / ring, unpadded blocks (n < 4096) -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mgs", "dmgs"])
@pytest.mark.parametrize("dims", [(100, 30), (63, 65)], ids=["n3000", "n4095"])
def test_masked_blocks_below_4096_rows(hip, dims, variant):
    """n = 3000 (93.75 rows of 32: the MASKED instantiations, the SpMV a launch of its own) and 4095 (odd: the last double2 is
    half padding, and the 4096 doubles of a column are one whole chunk of a four-row workgroup, so the unmasked kernels - the
    operator in the prologue, the blocked kernel from eight links on - take it).  12 steps, more than the ring's look-ahead;
    mgs with one double-sweep step, dmgs throughout."""
    m = 12
    c = dict(id="masked-%d-%s" % (dims[0] * dims[1], variant), op=("lap2d",) + dims, m=m,
             sweeps=_sw(m, at=(5,)) if variant == "mgs" else _sw(m, every=2), bars=_BAR_RING)
    for used in _run_case(c):
        expect_kernel(used["chain"] == m and used["n_chain_small"] >= m - 1, "a chain launch per step, the ring among them: %r" % (used,))
        expect_kernel(used["chain_fused"] == (0 if dims == (100, 30) else m), "SpMV apart / in the prologue: %r" % (used,))


# ---- the column ring k_mgs_chain_small, on one XCD and spread ------------------------------------------------------------
@pytest.mark.parametrize("form", ["prologue_value", "prologue_mask", "spmv"])
@pytest.mark.parametrize("dims", [(64, 64), (100, 144), (100, 1000), (100, 2100)], ids=["n4096", "n14400", "n100000", "n210000"])
def test_column_ring(hip, dims, form):
    """14 steps (one with two sweeps) with the blocked kernel off, so that the ring takes every step: look-ahead requests run
    past the last written column.  The operator in the ring's prologue in its value form and its mask form, and as a launch
    of its own (six diagonals)."""
    m = 14
    n = dims[0] * dims[1]
    kind = {"prologue_value": "lap2d_value", "prologue_mask": "lap2d", "spmv": "lap2d_6"}[form]
    c = dict(id="ring-%d-%s" % (n, form), op=(kind,) + dims, m=m, sweeps=_sw(m, at=(5,)), bars=_BAR_RING, set={"chain_blk": 0})
    for used in _run_case(c):
        # (the very first step of a banded operator is the three-pass Lanczos kernel: one link)
        expect_kernel(used["n_chain_small"] >= m - 1 and used["chain"] == m, "ring launches: %r" % (used,))
        expect_kernel(used["chain_fused"] == (0 if form == "spmv" else m), "operator in the prologue: %r" % (used,))
        expect_kernel((used["n_dia_mask"] > 0) == (form == "prologue_mask"), "mask-form launches: %r" % (used,))
        expect_kernel((used["n_chain_onex"] > 0) == (n <= 131072), "launches on one XCD: %r" % (used,))


# ---- the blocked kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,dims", [("blk", (260, 250)), ("blk2", (4000, 313))], ids=["blk-65000", "blk2-1252000"])
def test_blocked_kernels(hip, which, dims):
    """k_mgs_chain_blk (65,000 rows) and the eight-wave k_mgs_chain_blk2 (1,252,000 rows): 14 steps, those with eight links
    and more (k >= 7) through the blocked kernel, which reads four columns per sum and the Gram table's rows."""
    m = 14
    c = dict(id="%s-%d" % (which, dims[0] * dims[1]), op=("lap2d",) + dims, m=m, sweeps=_sw(m, at=(3,)), bars=_BAR_BLK)
    for used in _run_case(c):
        expect_kernel(used["n_chain_" + which] == m - 7, "blocked launches (steps k = 7 .. 13): %r" % (used,))


# ---- k_mgs_chain / _lds / _pf, 8 ... 40 rows per lane ----------------------------------------------------------------------
_N2 = {8: 700_000, 16: 1_500_000, 24: 2_800_000, 32: 3_900_000, 40: 5_000_000}     # double2 per vector (test_mgs_chain_every_register_shape)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("rows", [8, 16, 24, 32, 40])
def test_chain_register_shapes(hip, rows, cplx):
    """One size per register shape, real and complex, five steps (one with two sweeps), the SpMV a launch of its own."""
    m = 5
    n = _N2[rows] if cplx else 2 * _N2[rows]
    c = dict(id="chain-%d-%s" % (rows, "z" if cplx else "d"), op=("ztri" if cplx else "tri", n), m=m, sweeps=_sw(m, at=(3,)),
             bars=_BAR5(m), cplx=cplx, seed=rows)
    for used in _run_case(c):
        expect_kernel(used["chain"] == m and used["chain_fused"] == 0, "a chain launch per step: %r" % (used,))


@pytest.mark.parametrize("form", ["value", "mask"])
@pytest.mark.parametrize("rows,dims", [(16, (2000, 1500)), (24, (2800, 2000)), (40, (4000, 2500))], ids=["16", "24", "40"])
def test_chain_with_the_operator_in_the_prologue(hip, rows, dims, form):
    """16, 24 and 40 rows per lane with the 5-point operator computed in the chain's prologue, value form and mask form."""
    m = 5
    c = dict(id="chain-fused-%d-%s" % (rows, form), op=("lap2d_value" if form == "value" else "lap2d",) + dims, m=m,
             sweeps=_sw(m, at=(3,)), bars=_BAR5(m), seed=rows)
    for used in _run_case(c):
        expect_kernel(used["chain"] == m and used["chain_fused"] == m, "operator in the prologue of every step: %r" % (used,))
        expect_kernel((used["n_dia_mask"] > 0) == (form == "mask"), "mask-form launches: %r" % (used,))


# ---- 48 / 56 rows per lane -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12_000_000, 14_000_000])
def test_chain_long_vectors(hip, n):
    """12 M rows (48 rows per lane: k_mgs_chain_long, whose last store leaves its masking to a buffer descriptor) and 14 M rows
    (56 rows per lane, a part of w in LDS)."""
    m = 5
    c = dict(id="chain-long-%d" % n, op=("tri", n), m=m, sweeps=_sw(m, at=(3,)), bars=_BAR5(m), seed=48)
    for used in _run_case(c):
        expect_kernel(used["chain"] == m, "a chain launch per step: %r" % (used,))
        expect_kernel((used["n_chain_long"] >= m - 1) == (n == 12_000_000), "launches of the long kernel: %r" % (used,))


# ---- k_lanczos_fused ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobi", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("dims", [(300, 300), (4000, 2500)], ids=["n90000", "rows40"])
def test_lanczos_kernel(hip, dims, jacobi):
    """Six Lanczos steps through the three-pass kernel, plain and with the Jacobi diagonal (the P block), a deferred MINRES
    update riding along from step 2 on."""
    m = 6
    c = dict(id="lanczos-%d-%s" % (dims[0] * dims[1], "jacobi" if jacobi else "plain"), op=("lap2d",) + dims, m=m, sweeps=_sw(m),
             bars=_BAR5(m), lanczos=True, jacobi=jacobi, rides=True)
    for used in _run_case(c):
        expect_kernel(used["n_lanczos_fused"] == m, "three-pass launches: %r" % (used,))
        expect_kernel(used["n_minres_rides"] == m - 2, "MINRES updates carried by them: %r" % (used,))


# ---- the Jacobi two-block step (B = P != V) --------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("size", ["ring", "rows32"])
def test_jacobi_two_block_step(hip, size, cplx):
    """V = M P with the updates taken from P: a ring size (where the ring kernel itself does not apply) and 32 rows per lane."""
    m = 5
    if size == "ring":
        op = ("zlap2d" if cplx else "lap2d", 100, 1000)
    else:
        op = ("ztri", _N2[32]) if cplx else ("tri", 2 * _N2[32])
    c = dict(id="jacobi-%s-%s" % (size, "z" if cplx else "d"), op=op, m=m, sweeps=_sw(m, at=(3,)), bars=_BAR5(m), jacobi=True,
             cplx=cplx)
    for used in _run_case(c):
        # (complex steps with a preconditioner take the per-column kernels)
        expect_kernel(used["chain"] == (0 if cplx else m), "chain launches: %r" % (used,))


# ---- the panel form (gs_mode = 1) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cplx", [(8, False), (40, False), (48, False), (8, True), (40, True)],
                         ids=["8-real", "40-real", "48-real", "8-complex", "40-complex"])
def test_panel_form(hip, rows, cplx):
    """k_cgs_dots / k_cgs_update: all coefficients of a sweep from the same w.  In exact arithmetic the reference's numbers,
    and with an orthonormal basis of six columns within a few ulp of them."""
    m = 5
    n2 = 6_000_000 if rows == 48 else _N2[rows]
    n = n2 if cplx else 2 * n2
    c = dict(id="panel-%d-%s" % (rows, "z" if cplx else "d"), op=("ztri" if cplx else "tri", n), m=m, sweeps=_sw(m, at=(3,)),
             bars=_BAR5(m), cplx=cplx, gs_mode=1, seed=rows)
    for used in _run_case(c):
        expect_kernel(used["cgs_register"] > 0, "register-resident panel kernels: %r" % (used,))


# ---- the per-column fallback --------------------------------------------------------------------------------------------------
def test_link_kernels_with_the_chain_off(hip):
    """k_gs_link (kh_ctx_set "chain" 0) at 500,000 rows, the caller supplying w (A == NULL): W's other column stays poisoned."""
    m = 6
    c = dict(id="link-500000", op=("lap2d", 1000, 500), m=m, sweeps=_sw(m, at=(3,)), bars=_BAR5(m), set={"chain": 0},
             external_w=True)
    for used in _run_case(c):
        expect_kernel(used["chain"] == 0, "no chain launch: %r" % (used,))


# ---- a column offset -------------------------------------------------------------------------------------------------------------
def test_work_vector_in_the_second_column(hip):
    """wcol = 1 at 3 M rows (16 rows per lane), the operator in the prologue."""
    m = 5
    c = dict(id="wcol1-3000000", op=("lap2d", 2000, 1500), m=m, sweeps=_sw(m, at=(3,)), bars=_BAR5(m), wcol=1)
    for used in _run_case(c):
        expect_kernel(used["chain"] == m, "a chain launch per step: %r" % (used,))


def test_lanczos_window_that_does_not_start_at_column_zero(hip):
    """A Lanczos run in window coordinates: the live columns are k - 1 and k with k = 3, 4, ... (start = k > 0), columns 0
    and 1 of the block and everything behind the window are poisoned.  Columns 2 and 3 are the first two vectors of the
    extended-precision run (rounded to fp64); device step j is the reference's step j + 1."""
    from krypy_amd import _hip

    A = _operator("lap2d", 300, 300)
    n, m, c0 = A.shape[0], 6, 3
    v = _start_vector({}, n)
    Href, Vref, _ = po.arnoldi_longdouble(A, v, m + 1, 1, lanczos=True)
    res = {}
    for poisoned in (False, True):
        ctx = _hip.Context(0)
        try:
            Ad = ctx.csr(A)
            V, W = ctx.alloc(n, c0 + m + 2), ctx.alloc(n, 2)
            if poisoned:
                po.poison(V)
                po.poison(W)
            V.upload(c0 - 1, Vref[:, :2].astype(np.float64))
            H = np.zeros((m + 2, m + 1))
            H[1, 0] = float(Href[1, 0])
            lz0 = ctx.get("n_lanczos_fused")
            for j in range(1, m + 1):
                k = c0 + j - 1
                hcol = ctx.arnoldi_step(Ad, None, V, None, W, 0, k, k, 1, 0, float(H[j, j - 1]))
                H[j: j + 2, j] = hcol[k: k + 2]
                H[j - 1, j] = H[j, j - 1]
            res[poisoned] = dict(H=H, V=V.download(c0 - 1, m + 2), pad=[V.padding_nonzero(), W.padding_nonzero()],
                                 lz=ctx.get("n_lanczos_fused") - lz0)
        finally:
            ctx.close()
    clean, bad = res[False], res[True]
    po.bits_equal(bad["H"], clean["H"], "H")
    po.bits_equal(bad["V"], clean["V"], "V")
    assert bad["pad"] == [0, 0] and clean["pad"] == [0, 0], (bad["pad"], clean["pad"])
    herr, verr = _nrm(clean["H"][:, 1:] - Href[:, 1:]), _nrm(clean["V"] - Vref)
    print("FIGURES lanczos window: %.3e %.3e" % (herr / _nrm(Href), verr))
    assert herr <= 1e-12 * _nrm(Href[:, 1:])
    assert verr <= 1e-11 * np.sqrt(m)
    for r in (clean, bad):
        expect_kernel(r["lz"] == m, "three-pass launches: %r" % (r["lz"],))


# ---- an exact breakdown writes no NaN into the padding ------------------------------------------------------------------------
def _swap_identity(n, i):
    """The identity with rows i and i + 1 swapped, as CSR: the Krylov space of e_i has dimension 2."""
    idx = np.arange(n, dtype=np.int32)
    idx[i], idx[i + 1] = i + 1, i
    return sp.csr_matrix((np.ones(n), idx, np.arange(n + 1, dtype=np.int32)), shape=(n, n))


def _fixed_point_laplacian(nx, ny, i):
    """Five diagonals of the 5-point pattern with column i reduced to a diagonal entry 1: e_i is mapped to itself."""
    A = ref.laplace2d(nx, ny).tocsc()
    lo, hi = A.indptr[i], A.indptr[i + 1]
    A.data[lo:hi] = np.where(A.indices[lo:hi] == i, 1.0, 0.0)
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


@pytest.mark.parametrize("store", ["rows40", "rows48", "ring", "lanczos", "rows40_odd", "rows48_odd", "ring_odd"])
def test_exact_breakdown_leaves_the_padding_zero(hip, store):
    """h = 0 exactly, and the kernel divides by it: 0 / 0 in every lane behind the vector's end.  One unmasked size per store
    path, each with a last workgroup that is partly padding - 10 M rows (40 rows per lane, k_mgs_chain_lds), 12 M rows (48
    rows, k_mgs_chain_long), 100,000 rows (the ring), 90,000 rows (k_lanczos_fused, breakdown in step 0).  The last H entry
    is exactly 0, no padding word is non-zero, and a healthy sequence on the SAME blocks afterwards - column 0 uploaded,
    nothing else cleared - has the bits of that sequence on fresh blocks.  What the valid rows of the new column hold after
    the division is not asserted.

    The `_odd` variants (one row less) hold the contract as it is written down for an odd n (csrc/chain.h at CH_SLACK,
    DeviceVectors.__init__): row n shares its 16-byte row with row n - 1 and is stored with it as 0 / h, so after h == 0 that
    ONE word of V's padding is NaN like the valid rows of the column - measured: exactly one word, for each of the three
    store paths - and nothing else; it is gone once the column is cleared the way Arnoldi.advance clears it on an invariant
    subspace (kh_vec_zero), and the healthy sequence on the same blocks has the bits of fresh blocks either way."""
    from krypy_amd import _hip

    lanczos = store == "lanczos"
    odd = store.endswith("_odd")
    store = store[:-4] if odd else store
    n = {"rows40": 10_000_000, "rows48": 12_000_000, "ring": 100_000, "lanczos": 90_000}[store] - (1 if odd else 0)
    i = n // 3
    Abreak = _fixed_point_laplacian(300, 300, i) if lanczos else _swap_identity(n, i)
    healthy = dict(id="after-breakdown-" + store, op=("lap2d", 300, 300) if lanczos else ("tri", n), m=4, sweeps=_sw(4),
                   lanczos=lanczos)
    A = _operator(*healthy["op"])
    v = _start_vector(healthy, n)
    e = np.zeros(n)
    e[i] = 1.0
    counter = {"rows40": "chain_lds", "rows48": "n_chain_long", "ring": "n_chain_small", "lanczos": "n_lanczos_fused"}[store]
    ctx = _hip.Context(0)
    try:
        Ab = ctx.csr(Abreak)
        V, W = ctx.alloc(n, healthy["m"] + 2), ctx.alloc(n, 2)
        V.upload(0, e)
        if lanczos:
            c0 = _counters(ctx)
            h = ctx.arnoldi_step(Ab, None, V, None, W, 0, 0, 0, 1, 0)
            assert h[0] == 1.0
        else:
            h = ctx.arnoldi_step(Ab, None, V, None, W, 0, 0, 0, 1, 0)
            assert h[0] == 0.0 and h[1] == 1.0
            c0 = _counters(ctx)
            h = ctx.arnoldi_step(Ab, None, V, None, W, 0, 1, 0, 1, 0)
            assert h[0] == 1.0 and h[1] == 0.0
        took = _counters(ctx)[counter] - c0[counter]
        assert h[-1] == 0.0, h
        pads = [V.padding_nonzero(), W.padding_nonzero()]
        if odd:
            assert pads[0] <= 1 and pads[1] == 0, "non-zero padding words of V, W after the breakdown step (odd n): %r" % (pads,)
            assert np.isnan(V.download(2, 1)).all()      # (the step did divide by zero: the valid rows say so)
            keep = ctx.alloc(n, 1)
            keep.copy_from(0, V, 2)                      # the healthy sequence below runs on the column as the step left it
            V.zero(2, 1)
            pads = [V.padding_nonzero(), W.padding_nonzero()]
            assert pads == [0, 0], "non-zero padding words of V, W after clearing the column: %r" % (pads,)
            V.copy_from(2, keep, 0)
            del keep
        else:
            assert pads == [0, 0], "non-zero padding words of V, W after the breakdown step: %r" % (pads,)
        after = _sequence(ctx, healthy, A, v, None, False, blocks=(V, None, W))
        assert after["pad"] == [0, 0], after["pad"]
        del after["blocks"], V, W
    finally:
        ctx.close()
    ctx = _hip.Context(0)
    try:
        fresh = _sequence(ctx, healthy, A, v, None, False)
        del fresh["blocks"]
    finally:
        ctx.close()
    po.bits_equal(after["H"], fresh["H"], "H of the sequence after the breakdown against fresh blocks")
    po.bits_equal(after["V"], fresh["V"], "V of the sequence after the breakdown against fresh blocks")
    expect_kernel(took == 1, "the breakdown step took the kernel counted by %s: %r" % (counter, took))


# ---- solver level ---------------------------------------------------------------------------------------------------------------
def _solve(make):
    from krypy_amd import utils

    try:
        return make()
    except utils.ConvergenceError as e:
        return e.solver


def _fields(s):
    out = {"resnorms": np.array(s.resnorms, dtype=float), "xk": np.array(s.xk)}
    ar = getattr(s, "arnoldi", None)
    if ar is None:
        ar = getattr(s, "lanczos", None)
    if ar is not None:
        k = ar.iter
        out["H"] = np.array(ar.H[: k + 1, :k])
    if getattr(s, "store_arnoldi", False):
        out["V"] = np.array(s.V)
        out["H"] = np.array(s.H)
    return out


def _same_bits(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key in want:
        po.bits_equal(got[key], want[key], "%s: %s" % (what, key))


def _poisoned_solve_has_the_bits_of_the_clean_one(hip, make, what, expect_poisoned=True):
    """The solve outside the `with` on a flushed pool, then - its blocks parked - the same solve with every zero=False block
    poisoned on its way out of Context.alloc; the padding of every block still alive at the end."""
    gc.collect()
    hip._pool_flush()
    s = _solve(make)
    want = _fields(s)
    del s
    gc.collect()
    with po.poisoned_allocations(hip) as rec:
        s = _solve(make)
        got = _fields(s)
        hip.sync()
        pads = [blk.padding_nonzero() for blk in rec.live()]
        n_poisoned = rec.poisoned
    del s
    _same_bits(got, want, what)
    assert pads and not any(pads), "%s: non-zero padding words per live block: %r" % (what, pads)
    if expect_poisoned:
        assert n_poisoned > 0, "%s: no zero=False block was asked for" % what
    return want


@functools.lru_cache(maxsize=1)
def _system(nx, ny):
    A = ref.laplace2d(nx, ny)
    return A, np.random.default_rng(3).standard_normal(A.shape[0])


@pytest.mark.parametrize("cycle", ["c_cycle", "per_step"])
@pytest.mark.parametrize("ortho", ["mgs", "dmgs", "cgs2"])
@pytest.mark.parametrize("dims", [(100, 100), (400, 250), (1000, 1000), (1500, 1500)], ids=["1e4", "1e5", "1e6", "2.25e6"])
def test_gmres_on_poisoned_blocks(hip, monkeypatch, dims, ortho, cycle):
    """Gmres at N = 10^4 (ring), 10^5 (one XCD; mgs: the blocked kernel from eight links on), 10^6 (spread) and 2.25 M rows (16
    rows per lane, the operator in the chain's prologue), through kh_gmres_cycle and through the per-step loop."""
    from krypy_amd import linsys

    if cycle == "per_step":
        monkeypatch.setenv("KRYPY_AMD_GMRES_CYCLE", "0")
    A, b = _system(*dims)
    ls = linsys.LinearSystem(A, b)
    c0 = hip.get("n_cycle_steps")
    _poisoned_solve_has_the_bits_of_the_clean_one(
        hip, lambda: linsys.Gmres(ls, maxiter=20, tol=1e-30, ortho=ortho, store_arnoldi=True), "Gmres %s %s" % (ortho, cycle))
    expect_kernel((hip.get("n_cycle_steps") > c0) == (cycle == "c_cycle"), "steps inside kh_gmres_cycle: %r" % (cycle,))


def test_restarted_gmres_gets_the_previous_cycles_basis_back(hip):
    """Four cycles of GMRES(10): every cycle's basis is the block the cycle before parked."""
    from krypy_amd import linsys

    A, b = _system(400, 250)
    ls = linsys.LinearSystem(A, b)
    _poisoned_solve_has_the_bits_of_the_clean_one(
        hip, lambda: linsys.RestartedGmres(ls, maxiter=10, max_restarts=3, tol=1e-30), "RestartedGmres")


def test_a_basis_that_grows(hip, monkeypatch):
    """Arnoldi._grow: the basis starts with eight columns and moves to a larger zero=False block on demand."""
    from krypy_amd import linsys, utils

    monkeypatch.setattr(utils.Arnoldi, "_max_initial_cols", 8)
    A, b = _system(70, 70)
    ls = linsys.LinearSystem(A, b)
    want = _poisoned_solve_has_the_bits_of_the_clean_one(hip, lambda: linsys.Gmres(ls, tol=1e-9, store_arnoldi=True), "growing Gmres")
    assert want["V"].shape[1] > 16      # (it grew at least twice)


@pytest.mark.parametrize("n", [101, 100_001])
def test_invariant_subspace_with_an_odd_row_count(hip, n):
    """diag(1, ..., 1, 2, ..., 2) and b = ones: the Krylov space has dimension 2, the step that finds it divides by
    h = 0 (up to rounding) and the look-ahead steps behind it run on what it left.  With an odd n the word at row n of those
    columns is written along with row n - 1; Arnoldi clears the columns (padding included) before anything else sees them: no
    live block has a non-zero padding word, and the poisoned solve has the bits of the clean one."""
    from krypy_amd import linsys

    D = sp.diags(np.r_[np.ones(n // 2 + 1), 2 * np.ones(n // 2)]).tocsr()
    ls = linsys.LinearSystem(D, np.ones(n))
    want = _poisoned_solve_has_the_bits_of_the_clean_one(hip, lambda: linsys.Gmres(ls, tol=1e-12, maxiter=50), "invariant Gmres")
    assert len(want["resnorms"]) == 3


@pytest.mark.parametrize("kind", ["minres_window", "minres_stored", "cg"])
def test_minres_and_cg_on_poisoned_blocks(hip, kind):
    """Minres with the Jacobi preconditioner - windowed (the P block, the window moves, the deferred recurrences) and with the
    stored basis - and Cg."""
    from krypy_amd import linsys

    A, b = _system(300, 300)
    M = sp.diags(1.0 / np.linspace(3.0, 5.0, A.shape[0])).tocsr()
    if kind == "cg":
        make = lambda: linsys.Cg(linsys.LinearSystem(A, b, M=M, self_adjoint=True, positive_definite=True), tol=1e-30, maxiter=60)
    else:
        stored = kind == "minres_stored"
        make = lambda: linsys.Minres(linsys.LinearSystem(A, b, M=M, self_adjoint=True), tol=1e-30, maxiter=40 if stored else 150,
                                     store_arnoldi=stored)
    _poisoned_solve_has_the_bits_of_the_clean_one(hip, make, kind, expect_poisoned=kind != "cg")


def test_deflated_gmres_on_poisoned_blocks(hip):
    """DeflatedGmres with a 16-column U: the blocks of utils.qr and the projector inside the step."""
    from krypy_amd import deflation, linsys

    A, b = _system(300, 200)
    U = np.random.default_rng(4).standard_normal((A.shape[0], 16))
    ls = linsys.LinearSystem(A, b, self_adjoint=True)
    _poisoned_solve_has_the_bits_of_the_clean_one(
        hip, lambda: deflation.DeflatedGmres(ls, U=U, maxiter=30, tol=1e-30, store_arnoldi=True), "DeflatedGmres")


@pytest.mark.parametrize("kind", ["gmres", "minres_jacobi"])
def test_complex_solves_on_poisoned_blocks(hip, kind):
    from krypy_amd import linsys

    A, b = _system(300, 200)
    n = A.shape[0]
    rng = np.random.default_rng(8)
    bz = b + 1j * rng.standard_normal(n)
    if kind == "gmres":
        Az = (A + 0.3j * sp.diags(rng.standard_normal(n))).tocsr()
        make = lambda: linsys.Gmres(linsys.LinearSystem(Az, bz), maxiter=25, tol=1e-30, store_arnoldi=True)
    else:
        S = sp.diags(rng.standard_normal(n - 1) * 0.2, 1, shape=(n, n))
        Az = (A + 1j * (S - S.T)).tocsr()          # Hermitian
        M = sp.diags(1.0 / np.linspace(3.0, 5.0, n)).tocsr()
        make = lambda: linsys.Minres(linsys.LinearSystem(Az, bz, M=M, self_adjoint=True), maxiter=40, tol=1e-30)
    _poisoned_solve_has_the_bits_of_the_clean_one(hip, make, "complex " + kind)


def test_non_euclidean_inner_product_on_poisoned_blocks(hip):
    """ip_B given as an SPD matrix: the B V block beside the basis."""
    from krypy_amd import linsys

    A, b = _system(300, 200)
    B = sp.diags(np.linspace(0.5, 2.0, A.shape[0])).tocsr()
    ls = linsys.LinearSystem(A, b, ip_B=B)
    _poisoned_solve_has_the_bits_of_the_clean_one(hip, lambda: linsys.Gmres(ls, maxiter=25, tol=1e-30, store_arnoldi=True), "Gmres ip_B")


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("solver", ["gmres", "minres"])
def test_parked_blocks_full_of_nan_or_inf(hip, solver, value):
    """The scenario itself: a solve, its blocks parked, every parked block's rows overwritten with NaN / +Inf - what a solve
    that diverged leaves behind - and the same solve again: the bits of the first one."""
    import ctypes

    from krypy_amd import linsys

    A, b = _system(400, 250)
    M = sp.diags(1.0 / np.linspace(3.0, 5.0, A.shape[0])).tocsr()
    if solver == "gmres":
        make = lambda: linsys.Gmres(linsys.LinearSystem(A, b), maxiter=25, tol=1e-30, store_arnoldi=True)
    else:
        make = lambda: linsys.Minres(linsys.LinearSystem(A, b, M=M, self_adjoint=True), maxiter=100, tol=1e-30)
    gc.collect()
    hip._pool_flush()
    s = _solve(make)
    want = _fields(s)
    del s
    gc.collect()
    parked = 0
    for (rn, ncols), handles in hip._pool.items():
        fill = np.full(rn, value)
        for h in handles:
            for col in range(ncols):
                rc = hip._lib.kh_vec_upload(h, col, 1, fill.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), max(rn, 1))
                assert rc == 0
            parked += 1
    assert parked >= 2, "the first solve parked %d blocks" % parked
    s = _solve(make)
    got = _fields(s)
    del s
    _same_bits(got, want, "%s after parked blocks full of %r" % (solver, value))
