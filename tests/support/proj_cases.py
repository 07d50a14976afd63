"""One case table for the CPU and the GPU tests of the deflation projector (tests/test_proj_ref_host.py runs the rows that
fit a small machine through the NumPy twin, tests/test_gpu_proj.py all of them on the device), the seeded input
builders, and the driver that runs one row on a context - TEST INFRASTRUCTURE ONLY, importable without a GPU.

A length is an integer, or names an edge of a register shape of the chain-kernel geometry: ``c`` rows (of two doubles)
per lane serve ``(n + 1) // 2 <= ncu * c * 512``.  ``("first", c)`` is the smallest even n of the class (the boundary
plus 2; for 16 rows that is ``ncu / 2 + 1`` workgroups), ``("first", c, 3)`` an odd one next to it, ``("last", c)`` the
largest n of the class (every workgroup full: ``ncu`` workgroups, no padding row)."""
import collections

import numpy as np

ROWS = (4, 8, 16, 24, 32, 40, 48, 56)      # rows per lane of the register shapes
LANES = 512
HOST_LIMIT = 100003                        # rows up to this length run through the NumPy twin on any machine

Case = collections.namedtuple(
    "Case", "name path n d cplx iterations T WRH inplace acol ancols zcol zncols surplus w_is_v want_ya")


def case(name, path, n, d, cplx=False, iterations=2, T=True, WRH=True, inplace=False, acol=0, ancols=1, zcol=0, zncols=1,
         surplus=0, w_is_v=False, want_ya=True):
    return Case(name, path, n, d, cplx, iterations, T, WRH, inplace, acol, ancols, zcol, zncols, surplus, w_is_v, want_ya)


def resolve_n(n, ncu):
    if isinstance(n, tuple):
        c = ROWS.index(n[1])
        if n[0] == "first":
            return 2 * ncu * LANES * ROWS[c - 1] + (n[2] if len(n) > 2 else 2)
        assert n[0] == "last"
        return 2 * ncu * LANES * n[1]
    return int(n)


def class_of(n, ncu):
    """Rows per lane the chain-kernel geometry gives vectors of length n (0: none)."""
    if n < 2:
        return 0
    for c in ROWS:
        if (n + 1) // 2 <= ncu * c * LANES:
            return c
    return 0


_TW = ((True, True), (False, False), (True, False), (False, True))


def _paired(path, pairs, cplx):
    out = []
    for i, (n, d) in enumerate(pairs):
        T, WRH = _TW[i % 4]
        out.append(case("%s-n%d-d%d-it%d-T%d-WRH%d" % (path, n, d, 1 + i % 3, T, WRH), path, n, d, cplx=cplx,
                        iterations=1 + i % 3, T=T, WRH=WRH, want_ya=(i % 5 != 4)))
    return out


# a. the chunked kernels, real: chunk seams at d = 17 and 33, every n around the workgroup and block sizes
CHUNKED = _paired("chunked", [
    (1, 1), (1, 17), (2, 2), (2, 33), (63, 15), (63, 16), (64, 17), (64, 1), (65, 33), (65, 2), (257, 16), (257, 15),
    (4095, 17), (4095, 33), (4096, 1), (4096, 16), (4097, 2), (4097, 15), (4097, 33), (100003, 17), (100003, 16),
    (100003, 33), (4096, 2), (257, 1)], False) + [
    case("chunked-n4097-d257", "chunked", 4097, 257),              # k_small_matvec's stride loop
    case("chunked-n2049-d1024", "chunked", 2049, 1024),            # the stated limit; 1024 numbers through the staging buffer
    case("chunked-n2049-d1024-it1-noT", "chunked", 2049, 1024, iterations=1, T=False),
]

# e. the complex kernels: the 8 / 4 / 2 / 1 ladder (all four at d = 15), complex T and WRH
COMPLEX = _paired("complex", [
    (1, 1), (1, 9), (2, 2), (2, 15), (63, 3), (63, 16), (65, 7), (65, 17), (4097, 8), (4097, 15), (4097, 1), (100003, 9),
    (100003, 15), (100003, 16), (100003, 17), (4097, 3), (65, 2), (63, 7), (2, 8), (65, 15), (4097, 17), (100003, 7),
    (63, 9), (4097, 16)], True) + [
    case("complex-n600-d512", "complex", 600, 512, cplx=True),
    case("complex-n600-d512-it3-noWRH", "complex", 600, 512, cplx=True, iterations=3, WRH=False),
]

# b. call forms
FORMS = []
for _n in (4097, 70001):
    for _c in (False, True):
        _t = "forms-n%d-%s-" % (_n, "c128" if _c else "f64")
        FORMS += [
            case(_t + "inplace", "forms", _n, 5, cplx=_c, inplace=True, acol=1, ancols=3, zcol=1, zncols=3),
            case(_t + "columns", "forms", _n, 5, cplx=_c, acol=2, ancols=3, zcol=1, zncols=3),
            case(_t + "surplus", "forms", _n, 5, cplx=_c, surplus=2, iterations=3),
            case(_t + "w_is_v", "forms", _n, 5, cplx=_c, w_is_v=True, T=False, iterations=1),
        ]

# c. the one-launch kernel: one case per register shape, the edges of the 16-row class, ragged d and sweep counts
_S = ("first", 16)
REG = [
    case("reg-16rows-d16", "reg", _S, 16),
    case("reg-24rows-d8", "reg", ("first", 24), 8),
    case("reg-32rows-d8", "reg", ("first", 32), 8, inplace=True),
    case("reg-40rows-d4", "reg", ("first", 40), 4),
    case("reg-48rows-d4", "reg", ("first", 48), 4, T=False, WRH=True),
    case("reg-56rows-d4", "reg", ("first", 56), 4, T=True, WRH=False),
    case("reg-16rows-full-d8", "reg", ("last", 16), 8, iterations=3),
    case("reg-16rows-odd-d8", "reg", ("first", 16, 3), 8, iterations=1),
    case("reg-56rows-last-d4", "reg", ("last", 56), 4, iterations=1, inplace=True),
    case("reg-16rows-d1-it1", "reg", _S, 1, iterations=1, T=False, WRH=False),
    case("reg-16rows-d2-it3", "reg", _S, 2, iterations=3, T=True, WRH=False),
    case("reg-16rows-d8-it2", "reg", _S, 8, iterations=2, T=False, WRH=True, inplace=True),
    case("reg-16rows-d9-it1", "reg", _S, 9, iterations=1),
    case("reg-16rows-d15-it3", "reg", _S, 15, iterations=3, want_ya=False),
    case("reg-16rows-d16-it1", "reg", _S, 16, iterations=1, T=False, WRH=False),
]

# d. the panel passes without the one-launch kernel in front of them: d = 17, W is V (one block)
PANEL = [
    case("panel-40rows-even-d17-it1", "panel", ("first", 40), 17, iterations=1, w_is_v=True),
    case("panel-40rows-odd-d17-it2", "panel", ("first", 40, 3), 17, iterations=2, w_is_v=True),
]

TABLE = CHUNKED + COMPLEX + FORMS + REG + PANEL
assert len(set(c.name for c in TABLE)) == len(TABLE)


# ---- seeded inputs --------------------------------------------------------------------------------------------------
_SEED = 20260

def _uniform(rng, shape, cplx):
    """Zero mean, unit variance; complex: both parts, so no imaginary part vanishes."""
    x = (rng.random(shape) - 0.5) * np.sqrt(12.0)
    if cplx:
        x = x + 1j * (rng.random(shape) - 0.5) * np.sqrt(12.0)
    return x


def column(which, n, j, cplx):
    """Column j of W (which = 0) or V (1) at length n: random, scaled by 1 / sqrt(n); the same for every d."""
    return _uniform(np.random.default_rng([_SEED, which, n, j, int(cplx)]), n, cplx) / np.sqrt(n)


def block(which, n, ncols, cplx):
    out = np.empty((n, ncols), dtype=complex if cplx else float, order="F")
    for j in range(ncols):
        out[:, j] = column(which, n, j, cplx)
    return out


def small(which, d, cplx):
    """T (which = 2) or WRH (3): random, non-symmetric (complex: with imaginary parts), scaled by 1 / sqrt(d) so that a sweep
    does not blow the vector up and the errors stay measured against ||a||."""
    return _uniform(np.random.default_rng([_SEED, which, d, int(cplx)]), (d, d), cplx) / np.sqrt(d)


def vector(n, cplx, which=4):
    return _uniform(np.random.default_rng([_SEED, which, n, int(cplx)]), n, cplx)


Inputs = collections.namedtuple("Inputs", "W V T WRH a")


def inputs(c, n, blocks=None):
    """The host inputs of a row at length n.  ``blocks``: an optional ``(n, cplx) -> (W, V)`` cache of wide blocks whose
    leading columns are taken (generation dominates at the long lengths)."""
    if blocks is not None:
        Wb, Vb = blocks(n, c.cplx)
        W, V = Wb[:, :c.d], Vb[:, :c.d]
    else:
        W = block(0, n, c.d, c.cplx)
        V = W if c.w_is_v else block(1, n, c.d, c.cplx)
    if c.w_is_v:
        V = W
    return Inputs(W, V, small(2, c.d, c.cplx) if c.T else None, small(3, c.d, c.cplx) if c.WRH else None,
                  vector(n, c.cplx))


Run = collections.namedtuple("Run", "z ya Zh Z0 Ah A0 W0 V0 Wd Vd proj Ad Zd")


def run_case(ctx, c, inp, want_ya=None, keep=None):
    """One row on a context (the HIP one or its NumPy twin): blocks up, projector made, one call.  ``keep``: a previous
    ``Run`` of the same row whose device blocks and projector are used again (the source column is restored first).
    Returns ``Run``: ``z`` (the target column), ``ya``, the whole target block after and before the call, the source block
    after and before, and the device blocks."""
    n = inp.a.shape[0]
    dt = complex if c.cplx else float
    want_ya = c.want_ya if want_ya is None else want_ya
    rng = np.random.default_rng([_SEED, 9, n])
    A0 = _uniform(rng, (n, c.ancols), c.cplx)
    A0[:, c.acol] = inp.a
    Z0 = A0 if c.inplace else _uniform(rng, (n, c.zncols), c.cplx)
    if keep is None:
        def wide(B):
            if not c.surplus:
                return np.asarray(B, dtype=dt)
            out = np.full((n, c.d + c.surplus), np.nan, dtype=dt, order="F")
            out[:, :c.d] = B
            return out
        W0, V0 = wide(inp.W), np.asarray(inp.V, dtype=dt)
        Wd = ctx.upload(W0)
        Vd = Wd if c.w_is_v else ctx.upload(wide(inp.V))
        proj = ctx.proj_create(Wd, Vd, c.d, inp.T, inp.WRH, c.iterations)
        Ad = ctx.upload(np.asarray(A0, dtype=dt))
        Zd = Ad if c.inplace else ctx.upload(np.asarray(Z0, dtype=dt))
    else:
        W0, V0, Wd, Vd, proj, Ad, Zd = keep.W0, keep.V0, keep.Wd, keep.Vd, keep.proj, keep.Ad, keep.Zd
        Ad.upload(0, np.asarray(A0, dtype=dt))
        if not c.inplace:
            Zd.upload(0, np.asarray(Z0, dtype=dt))
    ya = ctx.proj_apply_complement(proj, Ad, c.acol, Zd, c.zcol, want_ya=want_ya)
    Zh = Zd.download()
    Ah = Zh if c.inplace else Ad.download()
    return Run(Zh[:, c.zcol].copy(), None if ya is None else np.array(ya), Zh, Z0, Ah, A0, W0, V0, Wd, Vd, proj, Ad, Zd)


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def check_untouched(c, run, blocks=True):
    """What a call must leave alone: every column of the target block but the target, the source block (but the target
    column of an in-place call), W and V - surplus NaN columns included - bit for bit (``blocks=False``: not downloaded, at
    the long lengths), and the padding of the target and of the bases."""
    dt = complex if c.cplx else float
    for j in range(run.Zh.shape[1]):
        if j != c.zcol:
            assert _same_bits(run.Zh[:, j], np.asarray(run.Z0[:, j], dtype=dt)), "column %d of the target block changed" % j
    if not c.inplace:
        assert _same_bits(run.Ah, np.asarray(run.A0, dtype=dt)), "the source block changed"
    if blocks:
        assert _same_bits(run.Wd.download(), np.asfortranarray(run.W0)), "W changed"
        if not c.w_is_v:
            assert _same_bits(run.Vd.download()[:, :c.d], np.asfortranarray(run.V0)), "V changed"
    assert run.Zd.padding_nonzero() == 0, "the padding of the target block is not zero"
    assert run.Wd.padding_nonzero() == 0 and run.Vd.padding_nonzero() == 0
