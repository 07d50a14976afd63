"""IDR(s) on the device: k_idr_dir / k_idr_orth / k_idr_omega / k_idr_rr bit for bit against tests/support/idrs_ref.py at
every position and edge, the stop word, ``idrs_run`` against the pieces, and whole solves on both paths of ``linsys.Idrs``."""
import math

import numpy as np
import pytest

from tests.support import bicgstab_cases as bc
from tests.support import idrs_cases as ic
from tests.support import idrs_ref as ref
from tests.support import poison
from tests.support.kernel_expect import expect_kernel

pytestmark = pytest.mark.gpu

L = ref.L
SENTINEL = -12345.6789          # in the columns a kernel must not touch (and must not read: it would show in the results)


def sum_bound(a, b):
    """2 n 2^-53 sum |a_i b_i|: the bound of tests/test_gpu_bicgstab.py (any summation order, doubled for the products)"""
    return 2.0 * a.size * 2.0 ** -53 * float(np.sum(np.abs(a.astype(np.longdouble) * b.astype(np.longdouble))))


def check_sum(got, a, b, what):
    if a.size <= 100000:
        want = math.fsum((a * b).tolist())
    else:                          # (the one long case: extended precision, as tests/test_gpu_bicgstab.py sums)
        want = float(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))
    err, bound = abs(got - want), sum_bound(a, b)
    print("%s: error %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, got, want, bound)


def random_scalars(s, seed):
    """a scalar block in mid-solve: lower-triangular M with a safe diagonal, f, om, rr"""
    rng = np.random.default_rng(seed)
    sc = ref.new_scalars()
    for i in range(s):
        for j in range(i):
            sc[L["M"] + i * ref.SM + j] = rng.standard_normal()
        sc[L["M"] + i * ref.SM + i] = 2.0 + rng.random()
    sc[L["F"]: L["F"] + s] = rng.standard_normal(s)
    sc[L["OM"]] = 0.625 + rng.random()
    return sc


class Dev(object):
    """a random state on the device: block H = [P | G | U | r | y | t] and the scalar block"""

    def __init__(self, hip, n, s, seed, sc):
        self.hip, self.n, self.s = hip, n, s
        self.H0 = np.asfortranarray(np.random.default_rng(seed).standard_normal((n, 3 * s + 3)))
        self.sc0 = sc.copy()
        self.iP, self.iG, self.iU, self.iR, self.iY, self.iT = 0, s, 2 * s, 3 * s, 3 * s + 1, 3 * s + 2

    def upload(self, sentinel=()):
        for c in sentinel:
            self.H0[:, c] = SENTINEL
        self.B = self.hip.upload(self.H0)
        self.SC = self.hip.upload(self.sc0)
        s = self.s
        return (self.B, 0, self.B, s, self.B, 2 * s, self.B, self.iR, self.B, self.iY, self.B, self.iT, self.SC, s)

    def download(self):
        assert not self.B.padding_nonzero()
        return self.B.download(), self.SC.download()[:, 0]

    def parts(self, H):
        s = self.s
        return H[:, :s], H[:, s: 2 * s], H[:, 2 * s: 3 * s], H[:, self.iR], H[:, self.iY], H[:, self.iT]

    def untouched(self, H, but=()):
        for c in range(H.shape[1]):
            if c not in but:
                poison.bits_equal(H[:, c], self.H0[:, c], "column %d is left as it was" % c)


def scalars_untouched(sc, sc0, but):
    keep = np.ones(L["REC"], dtype=bool)
    for name, width in but:
        keep[L[name]: L[name] + width] = False
    poison.bits_equal(sc[: L["REC"]][keep], sc0[: L["REC"]][keep], "scalars that the kernel does not store")


def check_dir(hip, n, s, k):
    d = Dev(hip, n, s, 100 * s + k, random_scalars(s, 7 * s + k))
    st = d.upload(sentinel=(d.iY, d.iT))
    hip.idrs_dir(st, k)
    H, sc = d.download()
    c, flags = ref.csolve(d.sc0, k, s)
    assert flags == 0 and sc[L["FLAGS"]] == 0.0 and sc[L["STOP"]] == 0.0
    poison.bits_equal(sc[L["C"] + k: L["C"] + s], np.array(c[k:]), "c of position %d" % k)
    scalars_untouched(sc, d.sc0, [("C", 8)])
    P, G, U, r, y, t = d.parts(d.H0)
    want = ref.dir_ref(r, G, U, k, s, list(sc[L["C"]: L["C"] + s]), float(sc[L["OM"]]))
    poison.bits_equal(H[:, d.iU + k], want, "u_%d (n = %d, s = %d)" % (k, n, s))
    d.untouched(H, but=(d.iU + k,))


def check_orth(hip, n, s, k):
    d = Dev(hip, n, s, 200 * s + k, random_scalars(s, 11 * s + k))
    st = d.upload(sentinel=tuple(range(d.iG + k, d.iG + s)))       # g_k and the later columns of G are not read
    rec = hip.idrs_orth(st, k, 1.0, 0.0)
    H, sc = d.download()
    P, G, U, r, y, t = d.parts(d.H0)
    for i in range(s):
        check_sum(float(sc[L["H"] + i]), P[:, i], t, "h_%d (n = %d, s = %d, k = %d)" % (i, n, s, k))
    before = d.sc0.copy()
    before[L["H"]: L["H"] + s] = sc[L["H"]: L["H"] + s]
    a, col, beta, fnew, flags = ref.asolve(before, k, s)
    assert flags == 0
    poison.bits_equal(sc[L["A"]: L["A"] + k], np.array(a), "a")
    poison.bits_equal(np.array([sc[L["M"] + i * ref.SM + k] for i in range(k, s)]), np.array(col), "M[k:, k]")
    assert sc[L["BETA"]] == beta
    poison.bits_equal(sc[L["F"] + k + 1: L["F"] + s], np.array(fnew), "f[k+1:]")
    g, u, rn, yn = ref.orth_ref(t, G, U, r, y, k, list(sc[L["A"]: L["A"] + k]), float(sc[L["BETA"]]))
    for name, col_i, want in (("g_k", d.iG + k, g), ("u_k", d.iU + k, u), ("r", d.iR, rn), ("y", d.iY, yn)):
        poison.bits_equal(H[:, col_i], want, "%s (n = %d, s = %d, k = %d)" % (name, n, s, k))
    d.untouched(H, but=(d.iG + k, d.iU + k, d.iR, d.iY))
    check_sum(rec[0], H[:, d.iR], H[:, d.iR], "rr")
    assert rec == (float(sc[L["RR"]]), col[0], float(d.sc0[L["F"] + k]), 0)
    assert sc[L["COUNT"]] == 1.0 and sc[L["STOP"]] == 0.0 and sc[L["FLAGS"]] == 0.0
    scalars_untouched(sc, d.sc0, [("H", 8), ("A", 8), ("BETA", 1), ("RR", 1), ("COUNT", 1), ("TMP", 1), ("F", 8), ("M", 64)])
    for i in range(s):                                             # of M only column k from row k down, of f only f[k+1:]
        for j in range(s):
            if not (j == k and i >= k):
                assert sc[L["M"] + i * ref.SM + j] == d.sc0[L["M"] + i * ref.SM + j]
    poison.bits_equal(sc[L["F"]: L["F"] + k + 1], d.sc0[L["F"]: L["F"] + k + 1], "f[:k+1]")
    return rec


def check_omega(hip, n, s):
    sc0 = random_scalars(s, 13 * s)
    d = Dev(hip, n, s, 300 * s, sc0)
    d.sc0[L["RR"]] = float(np.dot(d.H0[:, d.iR], d.H0[:, d.iR]))
    st = d.upload()
    rec = hip.idrs_omega(st, 1.0, 0.0)
    H, sc = d.download()
    P, G, U, r, y, t = d.parts(d.H0)
    check_sum(float(sc[L["THETA"]]), t, r, "theta (n = %d)" % n)
    check_sum(float(sc[L["PHI"]]), t, t, "phi (n = %d)" % n)
    om, flags = ref.omega_scalars(sc[L["THETA"]], sc[L["PHI"]], d.sc0[L["RR"]])
    assert flags == 0 and sc[L["OM"]] == om
    yn, rn = ref.omega_ref(r, t, y, float(sc[L["OM"]]))
    poison.bits_equal(H[:, d.iY], yn, "y (n = %d, s = %d)" % (n, s))
    poison.bits_equal(H[:, d.iR], rn, "r (n = %d, s = %d)" % (n, s))
    d.untouched(H, but=(d.iR, d.iY))
    for i in range(s):
        check_sum(float(sc[L["F"] + i]), P[:, i], rn, "f_%d (n = %d, s = %d)" % (i, n, s))
    poison.bits_equal(sc[L["F"]: L["F"] + s], sc[L["H"]: L["H"] + s], "f is the block dot")
    check_sum(rec[0], rn, rn, "rr")
    assert rec == (float(sc[L["RR"]]), float(sc[L["THETA"]]), float(sc[L["PHI"]]), 0)
    # (n = 1 without the correction: r - (t r / t t) t is exactly 0, and a residual of 0 meets every tolerance)
    assert sc[L["COUNT"]] == 1.0 and sc[L["STOP"]] == (1.0 if rec[0] == 0.0 else 0.0)
    scalars_untouched(sc, d.sc0, [("H", 8), ("F", 8), ("OM", 1), ("THETA", 2), ("RR", 1), ("COUNT", 1), ("TMP", 1), ("STOP", 1)])
    return abs(float(sc[L["THETA"]])) / math.sqrt(float(sc[L["PHI"]]) * d.sc0[L["RR"]])


@pytest.fixture
def reduce_blocks(hip):
    nb0 = hip.info()["reduce_blocks"]

    def tune(nb):
        if nb:
            hip.tune(reduce_blocks=nb)
        return hip

    try:
        yield tune
    finally:
        hip.tune(reduce_blocks=nb0)


# ---- the kernels, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [0, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4 * 256 + 3])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_kernels(reduce_blocks, s, n, nb):
    """every position k of every s: the vectors equal the reference's expressions with the device's own scalars, the small
    scalars equal the reference's forward substitutions, the sums are within the worst-case bound (nb = 3: three workgroups
    stride over the longer vectors)"""
    ctx = reduce_blocks(nb)
    for k in range(s):
        check_dir(ctx, n, s, k)
        check_orth(ctx, n, s, k)
    check_omega(ctx, n, s)


def test_omega_takes_both_branches(hip):
    """|rho| >= 0.7 at n = 1 (t and r are parallel), below it for long random vectors: the kappa correction"""
    assert check_omega(hip, 1, 2) >= ref.KAPPA
    assert check_omega(hip, 4 * 256 + 3, 2) < ref.KAPPA


def test_kernels_largest_grid(reduce_blocks):
    """reduce_blocks = 4096 and n = 8192 * 256 + 1: grid_lin would launch 8192 workgroups, the kernels here run on 4096 and
    their partial fills the slot to its last double"""
    ctx = reduce_blocks(4096)
    assert ctx.info()["reduce_blocks"] == 4096
    n = 8192 * 256 + 1
    check_dir(ctx, n, 2, 0)
    check_orth(ctx, n, 2, 1)
    check_omega(ctx, n, 2)


def test_same_call_same_bits(hip):
    n, s = 4 * 256 + 3, 4
    A = hip.csr(bc.convdiff(13, 79, 0.5, 0.25))
    out = []
    for _ in range(2):
        d = Dev(hip, n, s, 5, ref.new_scalars())
        d.H0[:, d.iG: d.iG + 2 * s] = 0.0
        d.H0[:, d.iY] = 0.0
        st = d.upload()
        hip.idrs_init(st)
        out.append((hip.idrs_run(A, st, 0, 11, 1.0, 0.0),) + d.download())
    assert out[0][0] == out[1][0] and len(out[0][0]) == 11
    poison.bits_equal(out[0][1], out[1][1], "vectors of the second run")
    poison.bits_equal(out[0][2], out[1][2], "scalars of the second run")


def test_pieces_are_the_run(hip):
    """dir + apply + orth ... + apply + omega leave the bits of one idrs_run over two cycles, for every operator kind"""
    n, s = 1027, 3
    Asp = bc.convdiff(13, 79, 1.0, 0.3)
    for kind in ("csr", "dense", "diag"):
        Amat = {"csr": lambda: hip.csr(Asp), "dense": lambda: hip.dense(Asp.toarray()),
                "diag": lambda: hip.diag(Asp.diagonal() + np.arange(n) / n)}[kind]()
        states = []
        for _ in range(2):
            d = Dev(hip, n, s, 9, ref.new_scalars())
            d.H0[:, d.iG: d.iG + 2 * s] = 0.0
            d.H0[:, d.iY] = 0.0
            states.append((d, d.upload()))
            hip.idrs_init(states[-1][1])
        (d0, st0), (d1, st1) = states
        recs = hip.idrs_run(Amat, st0, 0, 2 * (s + 1), 1.0, 0.0)
        mine = []
        for i in range(2 * (s + 1)):
            k = i % (s + 1)
            if k < s:
                hip.idrs_dir(st1, k)
                hip.apply(Amat, d1.B, d1.iU + k, d1.B, d1.iT)
                mine.append(hip.idrs_orth(st1, k, 1.0, 0.0))
            else:
                hip.apply(Amat, d1.B, d1.iR, d1.B, d1.iT)
                mine.append(hip.idrs_omega(st1, 1.0, 0.0))
        assert mine == recs, kind
        (H0, sc0), (H1, sc1) = d0.download(), d1.download()
        poison.bits_equal(H1, H0, "pieces against the run (%s)" % kind)
        poison.bits_equal(sc1[: L["STOP"]], sc0[: L["STOP"]], "scalars (%s)" % kind)      # (counter and records differ by design)


def test_zero_operator_clamps(hip):
    """A = 0: t = 0, h = 0, M_00 = 0: the pivot flag, beta clamped to 0, the step stops the run, nothing becomes inf or nan"""
    from krypy_amd import _hip
    n, s = 300, 2
    d = Dev(hip, n, s, 3, ref.new_scalars())
    d.H0[:, d.iG: d.iG + 2 * s] = 0.0
    d.H0[:, d.iY] = 0.0
    st = d.upload()
    hip.idrs_init(st)
    recs = hip.idrs_run(hip.diag(np.zeros(n)), st, 0, 3, 1.0, 0.0)
    H, sc = d.download()
    assert len(recs) == 1 and recs[0][3] == _hip.IDRS_PIVOT_ZERO and recs[0][1] == 0.0
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(sc))
    poison.bits_equal(H[:, d.iR], d.H0[:, d.iR], "beta = 0: r as it was")
    assert not np.any(H[:, d.iY]) and sc[L["STOP"]] == 1.0
    # position s on the same operator: theta = phi = 0, omega clamped and zero
    d2 = Dev(hip, n, s, 3, ref.new_scalars())
    st2 = d2.upload()
    hip.idrs_init(st2)
    rec = hip.idrs_run(hip.diag(np.zeros(n)), st2, s, 1, 1.0, 0.0)[0]
    assert rec[3] == _hip.IDRS_OMEGA_CLAMPED | _hip.IDRS_OMEGA_ZERO and rec[1] == 0.0 and rec[2] == 0.0
    H2, sc2 = d2.download()
    assert np.all(np.isfinite(H2)) and np.all(np.isfinite(sc2))
    poison.bits_equal(H2[:, d2.iR], d2.H0[:, d2.iR], "om = 0: r as it was")


def test_stop_word(hip):
    ic.case_stop_word(hip)


def test_argument_errors(hip):
    ic.case_abi_errors(hip)


# ---- the solver (the cases of tests/test_idrs_host.py on the device) ---------------------------------------------------
@pytest.mark.parametrize("s", [1, 3, 5])
def test_multiple_of_identity(hip, s):
    ic.case_multiple_of_identity(s)


def test_swap_breakdown(hip):
    ic.case_swap_breakdown()


@pytest.mark.parametrize("name,s", ic.WHOLE)
def test_whole_solve(hip, name, s):
    c0 = hip.get("n_idrs_steps")
    sol = ic.case_whole_solve(name, s)
    expect_kernel(hip.get("n_idrs_steps") - c0 == sol.iter, "every iteration inside an idrs_run call: %r, s = %d" % (name, s))


@pytest.mark.parametrize("name,s", ic.PAIRS)
def test_run_against_pieces(hip, name, s):
    c0 = hip.get("n_idrs_steps")
    pieces = ic.case_run_against_pieces(name, s, lambda: None)
    made = hip.get("n_idrs_steps") - c0
    # three solves through idrs_run, none of the pieces' iterations in the counter (a breakdown's step is recorded too)
    expect_kernel(made in (3 * pieces.iter, 3 * (pieces.iter + 1)), "idrs_run steps: %d for %d iterations" % (made, pieces.iter))


@pytest.mark.parametrize("side", ["Ml", "Mr"])
def test_generic_path(hip, side):
    c0 = hip.get("n_idrs_steps")
    ic.case_generic(side)
    expect_kernel(hip.get("n_idrs_steps") == c0, "a composite operator takes the pieces (%s)" % side)


def test_idr1_is_bicgstab(hip):
    ic.case_idr1_is_bicgstab()


def test_central(hip):
    ic.case_central()


def test_initial_guess(hip):
    ic.case_initial_guess()


def test_shapes(hip):
    ic.case_shapes()


def test_zero_rhs(hip):
    ic.case_zero_rhs()


def test_maxiter(hip):
    ic.case_maxiter()


def test_refusals(hip):
    ic.case_refusals()


def test_convenience(hip):
    ic.case_convenience()
