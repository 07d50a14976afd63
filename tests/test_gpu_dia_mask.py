"""The mask form of a constant-coefficient banded operator (csrc/kernels.h: dia_slot, k_dia_mask_fill).

An operator whose every diagonal holds ONE value (bitwise) on at most eight diagonals - the Laplacians of configs 2, 3
and 5 - is kept as one presence mask per row pair and nd values instead of the diagonal-major value copy.  A slot is
non-zero exactly where an entry exists, so every product and sum behind the slot values is the one the value copy gives:
the banded SpMV must match SciPy's csr_matvec bit for bit, and the fused chain / Lanczos prologues the separate SpMV
launch.  ``n_dia_mask`` counts the launches that read the mask form."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import krylov_ref as ref

from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

_DIA_ON = os.environ.get("KRYPY_AMD_SPMV_DIA", "") != "0"


def _lap1d(n):
    return sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")


def _operator(kind):
    """(operator, diagonals, mask form expected)"""
    if kind == "lap1d_min":          # the smallest banded size
        return _lap1d(3), 3, True
    if kind == "lap1d_odd":
        return _lap1d(30011), 3, True
    if kind == "lap2d_odd":          # neither whole workgroups nor an even row count
        return ref.laplace2d(97, 53), 5, True
    if kind == "lap2d_1025":
        return ref.laplace2d(41, 25), 5, True
    if kind == "lap3d_odd":
        return ref.laplace3d(23, 19, 17).tocsr(), 7, True
    if kind == "holes":              # constant values, entries deleted at random: an irregular mask
        A = ref.laplace2d(151, 139).tocoo()
        keep = np.random.default_rng(5).random(A.nnz) > 0.15
        A = sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=A.shape)
        A.sort_indices()
        return A, 5, True
    # constant but for ONE value one ulp off: the value copy serves
    A = ref.laplace2d(97, 53)
    A.data[A.nnz // 3] = np.nextafter(A.data[A.nnz // 3], 0.0)
    return A, 5, False


@pytest.mark.parametrize("kind", ["lap1d_min", "lap1d_odd", "lap2d_odd", "lap2d_1025", "lap3d_odd", "holes", "one_ulp_off"])
def test_banded_spmv_mask_form_bit_identical_to_scipy(hip, kind):
    A, nd, masked = _operator(kind)
    n = A.shape[0]
    rng = np.random.default_rng(17)
    x = rng.standard_normal((n, 3))
    Ad = hip.csr(A)
    if _DIA_ON:
        assert Ad.diagonals == nd
    X, Y = hip.upload(x), hip.alloc(n, 3)
    c0 = hip.get("n_dia_mask")
    hip.apply(Ad, X, 0, Y, 0, 1)                          # k_spmv_dia
    assert np.array_equal(Y.download()[:, 0], A.dot(x[:, 0])), kind
    c1 = hip.get("n_dia_mask")
    hip.apply(Ad, X, 0, Y, 0, 3)                          # k_spmm_dia
    assert np.array_equal(Y.download(), A.dot(x)), kind
    c2 = hip.get("n_dia_mask")
    b = rng.standard_normal((n, 1))
    R = hip.alloc(n, 1)
    nrm = hip.residual(Ad, hip.upload(b), 0, X, 1, R, 0)  # fused epilogue
    want = b[:, 0] - A.dot(x[:, 1])
    assert np.array_equal(R.download()[:, 0], want), kind
    assert abs(nrm - np.linalg.norm(want)) <= 1e-14 * np.linalg.norm(want)
    c3 = hip.get("n_dia_mask")
    if n >= 8:
        V, W = hip.alloc(n, 4), hip.alloc(n, 2)
        v0 = x[:, [0]] / np.linalg.norm(x[:, 0])
        V.upload(0, v0)
        h = hip.arnoldi_step(Ad, None, V, None, W, 0, 0, 0, 1, 0)
        w = A.dot(v0[:, 0])
        a0 = float(np.dot(v0[:, 0], w))
        assert abs(h[0] - a0) <= 1e-13 * np.linalg.norm(w)
    c4 = hip.get("n_dia_mask")
    on = masked and _DIA_ON
    expect_kernel((c1 - c0, c2 - c1, c3 - c2) == ((1, 1, 1) if on else (0, 0, 0)),
                  "mask-form launches of SpMV / SpMM / residual: %r" % ((kind, c1 - c0, c2 - c1, c3 - c2),))
    expect_kernel((c4 - c3 >= 1) if (on and n >= 8) else (c4 == c3), "mask-form launches of the Arnoldi step: %r" % ((kind, c4 - c3),))


def _context(fused_spmv):
    from krypy_amd import _hip

    want = {"KRYPY_AMD_MGS_CHAIN": "1", "KRYPY_AMD_CHAIN_SPMV": "1" if fused_spmv else "0"}
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        return _hip.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# 16, 24, 40 and 48 rows per lane of the chain kernels (256 compute units)
@pytest.mark.parametrize("shape", [("lap2d", 1700, 1500), ("lap2d", 2400, 2300), ("lap2d", 3300, 3000), ("lap3d", 223, 0)])
def test_fused_prologues_read_the_mask_form(hip, shape):
    """MGS (k_mgs_chain_lds / k_mgs_chain_long) and Lanczos with Jacobi (k_lanczos_fused, config 3's kernel) with the
    operator in the prologue: H and the vectors bit for bit those of the separate SpMV launch (chain_spmv = 0)."""
    kind, a, b_ = shape
    A = ref.laplace2d(a, b_) if kind == "lap2d" else ref.laplace3d(a).tocsr()
    n = A.shape[0]
    v = np.random.default_rng(7).standard_normal(n)
    dj = np.linspace(0.5, 1.5, n)
    m = 4
    out = []
    for fused in (True, False):
        ctx = _context(fused)
        Ad, Md = ctx.csr(A), ctx.diag(dj)
        res = {}
        for name, use_m, lanczos in (("mgs", False, False), ("lanczos_jacobi", True, True)):
            c0 = ctx.get("n_dia_mask")
            f0 = ctx.counters()["chain_fused"]
            V, W = ctx.alloc(n, m + 1), ctx.alloc(n, 2)
            P = ctx.alloc(n, m + 1) if use_m else None
            if use_m:
                nrm = np.sqrt(np.dot(v, dj * v))
                P.upload(0, v / nrm)
                V.upload(0, dj * v / nrm)
            else:
                V.upload(0, v / np.linalg.norm(v))
            H = np.zeros((m + 1, m))
            for k in range(m):
                start = k if lanczos else 0
                hk = float(H[k, k - 1]) if (lanczos and k > 0) else 0.0
                hcol = ctx.arnoldi_step(Ad, Md if use_m else None, V, P, W, 0, k, start, 1, 0, hk)
                H[start: k + 2, k] = hcol[start: k + 2]
            res[name] = (H, V.download(), P.download() if use_m else np.zeros(1))
            dm = ctx.get("n_dia_mask") - c0
            df = ctx.counters()["chain_fused"] - f0
            if _DIA_ON:
                expect_kernel(df == (m if fused else 0), "fused chain launches: %r" % ((name, fused, df),))
                expect_kernel(dm >= m, "every step read the mask form: %r" % ((name, fused, dm),))
            del V, W, P
        out.append(res)
        ctx.close()
    for name in out[0]:
        (Hf, Vf, Pf), (Hs, Vs, Ps) = out[0][name], out[1][name]
        assert np.array_equal(Hf, Hs), (name, shape)
        assert np.array_equal(Vf, Vs), (name, shape)
        assert np.array_equal(Pf, Ps), (name, shape)


@pytest.fixture
def loop_ctx(hip):
    """A 1-rank communicator in forced multi-rank mode with the loopback halo (tests/test_gpu_halo_loopback.py)."""
    from krypy_amd import _hip

    os.environ["KRYPY_AMD_FORCE_MULTI"] = "1"
    try:
        ctx = _hip.Context(0)
        ctx.comm_init(0, 1, ctx.comm_unique_id())
    finally:
        del os.environ["KRYPY_AMD_FORCE_MULTI"]
    ctx.set("halo_loopback", 1)
    yield ctx
    ctx.close()


def test_periodic_slab_halo_in_the_launch_reads_the_mask_form(loop_ctx):
    """A shard of the 7-point Laplacian (ghost rows, dia_rebuild_for_halo) takes the mask form; with the halo inside the
    banded launch (k_spmv_dia<..., XH>) its product is SciPy's on the tripled operator, bit for bit."""
    from krypy_amd import dist

    ctx = loop_ctx
    T = lambda k: sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])     # noqa: E731
    I = sp.identity                                                                               # noqa: E731,E741
    Abig = (sp.kron(I(60), sp.kron(I(33), T(37))) + sp.kron(I(60), sp.kron(T(33), I(37))) +
            sp.kron(T(60), sp.kron(I(33), I(37)))).tocsr()
    Abig.sort_indices()
    n = 37 * 33 * 20
    A_local, nrp, nrn = dist.localize_columns(Abig[n:2 * n], n, 3 * n)
    Ad = ctx.csr(A_local, n_cols=A_local.shape[1])
    ctx.set_halo(Ad, nrn, nrp, nrp, nrn)
    if not _DIA_ON:
        pytest.skip("no banded form of the shard (KRYPY_AMD_SPMV_DIA=0)")
    assert Ad.diagonals == 7
    ctx.xh_export(Ad)
    ctx.xh_attach(Ad, None, 0, 0, None, 0, self_loop=True)
    ctx.xh_enable(Ad, True)
    rng = np.random.default_rng(23)
    c0, x0 = ctx.get("n_dia_mask"), ctx.get("n_halo_xh")
    for rep in range(4):
        x = rng.standard_normal(n)
        X, Y = ctx.upload(x), ctx.alloc(n, 1)
        ctx.apply(Ad, X, 0, Y, 0, 1)
        assert np.array_equal(Y.download()[:, 0], Abig[n:2 * n].dot(np.tile(x, 3))), rep
    expect_kernel(ctx.get("n_halo_xh") - x0 == 4, "the halo inside the launch: %r" % (ctx.get("n_halo_xh") - x0,))
    expect_kernel(ctx.get("n_dia_mask") - c0 == 4, "mask-form launches: %r" % (ctx.get("n_dia_mask") - c0,))
    ctx.xh_detach(Ad)
