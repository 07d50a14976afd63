"""The projector reference (tests/support/proj_ref.py) and the case table (tests/support/proj_cases.py) checked on the
CPU: the reference is exact where the result is representable, its extended run is orthogonal at the extended epsilon,
``assert_matches`` rejects a list of wrong projectors, and every table row of a modest length passes through the NumPy
twin of the device context - table, builders and bars are tried before anything reaches a GPU."""
import numpy as np
import pytest

from tests.support import proj_cases as pc
from tests.support import proj_ref as pr
from tests.support.numpy_context import NumpyContext


@pytest.mark.parametrize("cplx", [False, True])
def test_reference_is_exact_on_small_integers(cplx):
    """n = 8, d = 2, two sweeps, integer W, V, T, WRH and a: every intermediate is a small (Gaussian) integer, so the
    extended run, the float64 run and integer arithmetic agree exactly."""
    rng = np.random.default_rng(5)

    def ints(shape):
        x = rng.integers(-3, 4, shape)
        return x + 1j * rng.integers(-3, 4, shape) if cplx else x

    n, d = 8, 2
    W, V, T, WRH, a = ints((n, d)), ints((n, d)), ints((d, d)), ints((d, d)), ints(n)
    z = a.copy()
    ya = None
    for it in range(2):          # Python integers: exact
        c = [sum(int(np.real(np.conj(W[i, j]) * z[i])) + 1j * int(np.imag(np.conj(W[i, j]) * z[i])) for i in range(n))
             for j in range(d)]
        if it == 0:
            ya = [sum(WRH[i, j] * c[j] for j in range(d)) for i in range(d)]
        cp = [sum(T[i, j] * c[j] for j in range(d)) for i in range(d)]
        z = np.array([z[i] - sum(V[i, j] * cp[j] for j in range(d)) for i in range(n)])
    assert np.any(z != a) and np.any(np.array(ya) != 0)
    for dtype in (np.longdouble, np.float64):
        gz, gya = pr.complement(W, V, d, T, WRH, 2, a, dtype=dtype)
        assert gz.dtype == (pr._working_type(dtype, cplx))
        assert np.array_equal(gz.astype(complex), np.asarray(z, dtype=complex))
        assert np.array_equal(gya.astype(complex), np.asarray(ya, dtype=complex))
    # T and WRH of None: the identity
    gz, gya = pr.complement(W, V, d, None, None, 1, a)
    c = np.conj(W).T.dot(a)
    assert np.array_equal(gya.astype(complex), c.astype(complex))
    assert np.array_equal(gz.astype(complex), (a - V.dot(c)).astype(complex))


@pytest.mark.parametrize("cplx", [False, True])
def test_extended_run_is_orthogonal_at_the_extended_epsilon(cplx):
    """W = V orthonormal (a float64 QR: orthonormal to 1e-16), T = None, three sweeps - each one squares the defect - :
    W^H z of the extended result is rounding of the LAST sweep alone.  Each of its d dots of n products carries at most
    log2(n) + 1 roundings of the pairwise sum and one of the product, on terms of total size <= ||w|| ||z||; the float64
    run of the same thing sits three orders above that bound."""
    n, d = 4097, 7
    rng = np.random.default_rng(11)
    X = rng.standard_normal((n, d)) + (1j * rng.standard_normal((n, d)) if cplx else 0.0)
    Q = np.linalg.qr(X)[0]
    a = pc.vector(n, cplx)
    eps_ld = float(np.finfo(np.longdouble).eps)
    wide = np.clongdouble if cplx else np.longdouble

    def defect(z):
        z = z.astype(wide)
        return float(pr._norm(np.array([(np.conj(Q[:, j].astype(wide)) * z).sum() for j in range(d)])))

    z, ya = pr.complement(Q, Q, d, None, None, 3, a)
    bound = 2.0 * (np.log2(n) + 2.0) * eps_ld * np.sqrt(d) * float(pr._norm(a)) * (2.0 if cplx else 1.0)
    assert defect(z) <= bound, (defect(z), bound)
    z64, _ = pr.complement(Q, Q, d, None, None, 3, a, dtype=np.float64)
    # the yardstick is a float64 run, not the extended one in disguise: its epsilon is 2048 times the extended one
    assert defect(z64) > 64.0 * defect(z), (defect(z64), defect(z))
    assert pr.errors((z64, None), (z, ya), pr._norm(a))["z"] < 1e-15


def _mutant(W, V, d, T, WRH, iterations, a, kind):
    """The formula in float64 NumPy with one thing wrong."""
    cplx = np.iscomplexobj(a)
    z = np.array(a)
    ya = None
    sweeps = iterations - 1 if kind == "one sweep fewer" else iterations
    Tm = T.T if kind == "T transposed" else (np.conj(T) if kind == "T conjugated" else T)
    for it in range(sweeps):
        Wd = W[:, :d]
        if kind == "float32 dots":
            c = np.array([np.sum((np.conj(Wd[:, j]) * z).astype(np.complex64 if cplx else np.float32), dtype=np.complex64
                                 if cplx else np.float32) for j in range(d)]).astype(z.dtype)
        elif kind == "W not conjugated":
            c = Wd.T.dot(z)
        else:
            c = np.conj(Wd).T.dot(z)
        if it == 0 or kind == "ya of the last sweep":
            ya = c.copy() if kind == "WRH ignored" else WRH.dot(c)
        cp = Tm.dot(c)
        if kind == "one column of V skipped":
            cp = cp.copy()
            cp[d // 2] = 0.0
        z = z - V[:, :d].dot(cp)
    return z, ya


_MUTANTS = ["one sweep fewer", "T transposed", "ya of the last sweep", "WRH ignored", "one column of V skipped",
            "float32 dots", "one element moved", "W not conjugated", "T conjugated"]


@pytest.mark.parametrize("cplx", [False, True])
def test_assert_matches_rejects_the_mutants(cplx):
    """One fixed case (n = 4097, d = 7, two sweeps, T and WRH given): the plain float64 formula passes, each mutant of it
    is rejected.  'W not conjugated' and 'T conjugated' are mutants of complex data only."""
    n, d = 4097, 7
    c = pc.case("mutants", "host", n, d, cplx=cplx)
    inp = pc.inputs(c, n)
    ref = pr.complement(inp.W, inp.V, d, inp.T, inp.WRH, 2, inp.a)
    yard = pr.complement(inp.W, inp.V, d, inp.T, inp.WRH, 2, inp.a, dtype=np.float64)
    scale = pr._norm(inp.a)
    good = _mutant(inp.W, inp.V, d, inp.T, inp.WRH, 2, inp.a, "none")
    errs, bars = pr.assert_matches(good, ref, yard, d, scale)
    assert set(errs) == {"z", "ya"}
    for kind in _MUTANTS:
        if kind in ("W not conjugated", "T conjugated") and not cplx:
            continue
        if kind == "one element moved":
            z = good[0].copy()
            z[n // 3] += 64.0 * bars["z"] * float(scale)
            bad = (z, good[1])
        else:
            bad = _mutant(inp.W, inp.V, d, inp.T, inp.WRH, 2, inp.a, kind)
        with pytest.raises(AssertionError):
            pr.assert_matches(bad, ref, yard, d, scale)
    nan = good[0].copy()
    nan[5] = np.nan
    with pytest.raises(AssertionError):
        pr.assert_matches((nan, good[1]), ref, yard, d, scale)
    with pytest.raises(AssertionError):
        pr.assert_matches((good[0], good[1] * np.nan), ref, yard, d, scale)
    # ya not requested: z alone is compared
    errs, _ = pr.assert_matches((good[0], None), ref, yard, d, scale)
    assert set(errs) == {"z"}


def test_table_covers_what_it_promises():
    ncu = 256
    assert pc.resolve_n(("first", 16), ncu) == 2097154 and pc.class_of(2097154, ncu) == 16 and pc.class_of(2097152, ncu) == 8
    assert pc.resolve_n(("last", 56), ncu) == 14680064 and pc.class_of(14680064, ncu) == 56 and pc.class_of(14680065, ncu) == 0
    assert pc.class_of(pc.resolve_n(("first", 40, 3), ncu), ncu) == 40 and pc.class_of(1, ncu) == 0
    for path, cases in (("chunked", pc.CHUNKED), ("complex", pc.COMPLEX)):
        assert {c.iterations for c in cases} == {1, 2, 3}
        assert {(c.T, c.WRH) for c in cases} == {(True, True), (True, False), (False, True), (False, False)}
        assert {c.want_ya for c in cases} == {True, False}
        assert all(c.path == path and c.cplx == (path == "complex") for c in cases)
    assert {c.n for c in pc.CHUNKED} >= {1, 2, 63, 64, 65, 257, 4095, 4096, 4097, 100003}
    assert {c.d for c in pc.CHUNKED} == {1, 2, 15, 16, 17, 33, 257, 1024}
    assert {c.n for c in pc.COMPLEX} >= {1, 2, 63, 65, 4097, 100003}
    assert {c.d for c in pc.COMPLEX} == {1, 2, 3, 7, 8, 9, 15, 16, 17, 512}
    assert {pc.class_of(pc.resolve_n(c.n, ncu), ncu) for c in pc.REG} == {16, 24, 32, 40, 48, 56}


_HOST_ROWS = [c for c in pc.TABLE if not isinstance(c.n, tuple) and c.n <= pc.HOST_LIMIT]


@pytest.mark.parametrize("c", _HOST_ROWS, ids=[c.name for c in _HOST_ROWS])
def test_table_row_through_the_numpy_twin(c):
    """The row on the NumPy twin of the device context: numbers within the bars, and the call-form contracts the GPU test
    asserts (other columns of the target, the source, W and V untouched)."""
    ctx = NumpyContext()
    inp = pc.inputs(c, c.n)
    ref = pr.complement(inp.W, inp.V, c.d, inp.T, inp.WRH, c.iterations, inp.a)
    yard = pr.complement(inp.W, inp.V, c.d, inp.T, inp.WRH, c.iterations, inp.a, dtype=np.float64)
    run = pc.run_case(ctx, c, inp)
    assert (run.ya is not None) == c.want_ya
    pr.assert_matches((run.z, run.ya), ref, yard, c.d, pr._norm(inp.a))
    pc.check_untouched(c, run)
