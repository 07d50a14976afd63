"""The IDR(s) cases that tests/test_idrs_host.py (on the NumPy double) and tests/test_gpu_idrs.py (on the device) both run -
TEST INFRASTRUCTURE ONLY.  Every function works on whatever context is installed."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bicgstab_cases as bc
from tests.support import bicgstab_ref
from tests.support import idrs_ref as ref

TOL = 1e-8
# resnorms[1:9] against solve_ref(numpy.dot).  Measured on the CPU between the four summation orders of idrs_ref, s in
# {1, 2, 4, 8}, on every system of SYSTEMS and on scaled_system: at most 1.53e-11 (cd37x23-rng, s = 2; 1.19e-11 for s = 4 on
# cd24-ones); tests/test_idrs_host.py holds the reference to 2e-11.  Two orders of magnitude on top, because the device's order
# is a fifth one.
RTOL = 2e-9
# IDR(1) with shadow = r0 against BiCGStab, the residual norms after every second iteration of the first four cycles: measured
# between idrs_ref and bicgstab_ref in each of the four orders on scaled_system at most 6.8e-16; two orders of magnitude on top.
RTOL_BICGSTAB = 1e-13


def central(nx, ny, cx, cy):
    """Five-point diffusion plus CENTRAL-difference convection on an nx x ny grid, row-major:
    kron(I_ny, Tx) + kron(Ty, I_nx), Tx = tridiag(-1 - cx, 2, -1 + cx), Ty likewise with cy.  CSR."""
    def tri(m, c):
        return sp.diags([np.full(m - 1, -1.0 - c), np.full(m, 2.0), np.full(m - 1, -1.0 + c)], [-1, 0, 1])
    return sp.csr_matrix(sp.kron(sp.identity(ny), tri(nx, cx)) + sp.kron(tri(ny, cy), sp.identity(nx)))


SYSTEMS = {
    "cd24-ones": (lambda: bc.convdiff(24, 24, 0.5, 0.25), "ones"),
    "cd37x23-rng": (lambda: bc.convdiff(37, 23, 1.0, 0.3), "rng"),
    "cd40-ones": (lambda: bc.convdiff(40, 40, 20.0, 10.0), "ones"),
    "central32-ones": (lambda: central(32, 32, 4.0, 2.0), "ones"),
}
# whole solves: every system with s = 1, 4, 8 - but central32 with s = 1, where the reference's own four orders take 435 to
# 890 iterations (IDR(1) is BiCGStab, which does not like this system): the 15 % cap cannot hold there
WHOLE = [(name, s) for name in sorted(SYSTEMS) for s in (1, 4, 8) if (name, s) != ("central32-ones", 1)]
# run against pieces
PAIRS = [(name, s) for name in ("cd24-ones", "cd37x23-rng", "central32-ones") for s in (1, 4, 8)]


@functools.lru_cache(maxsize=None)
def system(name):
    make, kind = SYSTEMS[name]
    A = make()
    return A, bc.rhs(A.shape[0], kind)


@functools.lru_cache(maxsize=None)
def reference(name, s):
    """solve_ref on a named system in the four summation orders (computed once per process, never modified)"""
    A, b = system(name)
    return {o: ref.solve_ref(A, b, TOL, 4 * A.shape[0], s=s, dot=d) for o, d in ref.DOTS.items()}


def order_spread(name, s):
    """largest relative difference of resnorms[1:9] between the four summation orders of the reference"""
    v = np.array([r.resnorms[1:9] for r in reference(name, s).values()])
    return float(np.max((v.max(axis=0) - v.min(axis=0)) / v.min(axis=0)))


def solve(A, b, **kw):
    from krypy_amd import linsys
    lskw = {k: kw.pop(k) for k in ("Ml", "Mr") if k in kw}
    kw.setdefault("tol", TOL)
    return linsys.Idrs(linsys.LinearSystem(A, b, **lskw), **kw)


class WithoutRun(object):
    """the installed context with ``idrs_run`` hidden: ``linsys.Idrs`` takes the pieces, on the same device matrix, with
    the same residual kernel around the iteration"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        if name == "idrs_run":
            raise AttributeError(name)
        return getattr(self._ctx, name)


def solve_pieces(A, b, **kw):
    from krypy_amd import linsys
    kw.setdefault("tol", TOL)
    ls = linsys.LinearSystem(A, b)
    ls._ctx = WithoutRun(ls._ctx)
    return linsys.Idrs(ls, **kw)


# ---- edges ----------------------------------------------------------------------------------------------------------------
def case_multiple_of_identity(s=3):
    """A = 2 I: u_0 = r, t = 2 r, h = 2 f exactly, beta = 1/2, r = 0 after ONE iteration, x = b / 2 exactly"""
    b = np.array([1.0, -2.0, 3.0, 0.5, 4.0])
    sol = solve(sp.csr_matrix(2.0 * sp.identity(5)), b, s=s)
    assert sol.iter == 1
    assert np.array_equal(sol.xk.reshape(-1), b / 2)
    assert sol.resnorms[-1] == 0.0
    assert len(sol.idrs_trace) == 1 and sol.idrs_trace[0][:3] == (0, 0, 0.0) and sol.idrs_trace[0][-1] == 0


def case_swap_breakdown():
    """A = [[0, 1], [1, 0]], b = e_1, shadow = r0 = e_1: M_00 = <e_1, A e_1> = 0 in the first iteration"""
    from krypy_amd import _hip, utils
    with pytest.raises(utils.ConvergenceError, match=r"IDR\(s\) breakdown in iteration 0 \(M_kk is zero") as ei:
        solve(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), np.array([1.0, 0.0]), s=1, shadow=np.array([[1.0], [0.0]]))
    assert "flags %d" % _hip.IDRS_PIVOT_ZERO in str(ei.value)
    sol = ei.value.solver
    assert np.all(np.isfinite(sol.xk)) and sol.xk.shape == (2, 1)
    assert len(sol.idrs_trace) == 1 and sol.idrs_trace[0][-1] == _hip.IDRS_PIVOT_ZERO


# ---- whole solves -----------------------------------------------------------------------------------------------------------
def case_whole_solve(name, s, **kw):
    A, b = system(name)
    refs = reference(name, s)
    sol = solve(A, b, s=s, **kw)
    assert sol.resnorms[-1] <= TOL
    assert bc.relres(A, sol.xk, b) <= TOL * (1 + 1e-6)
    want = np.array(refs["numpy"].resnorms[1:9])
    got = np.array(sol.resnorms[1:9])
    print("%s s = %d: iter %d (reference %s), resnorms[1:9] max rel diff %.3e" % (
        name, s, sol.iter, sorted(r.iter for r in refs.values()), np.max(np.abs(got - want) / want)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    assert sol.iter <= math.ceil(1.15 * max(r.iter for r in refs.values()))
    return sol


def _solve_or_error(A, b, how=solve, **kw):
    from krypy_amd import utils
    try:
        return how(A, b, **kw), None
    except utils.ConvergenceError as e:
        return e.solver, str(e)


def case_run_against_pieces(name, s, run_calls):
    """idrs_run with 1, s + 1 and 64 steps per call and the pieces: identical resnorms, identical xk bits;
    ``run_calls()``: how many idrs_run calls the context has seen (None where it does not count them).  (central32-ones with s = 1 is BiCGStab on a system it
    does not like: the reference stagnates there for hundreds of iterations and, in numpy.dot's order, ends in a breakdown -
    whatever happens has to happen on both paths alike, message included.)"""
    A, b = system(name)
    pieces, err = _solve_or_error(A, b, how=solve_pieces, s=s)
    assert err is not None or pieces.resnorms[-1] <= TOL
    for spc in (1, s + 1, 64):
        before = run_calls()
        sol, err_run = _solve_or_error(A, b, s=s, steps_per_call=spc)
        assert sol.resnorms == pieces.resnorms, (name, s, spc)
        assert np.array_equal(sol.xk, pieces.xk), (name, s, spc)
        assert err_run == err and sol.iter == pieces.iter and list(sol.idrs_trace) == list(pieces.idrs_trace)
        if err is None and before is not None:
            # every call but the last does spc iterations; the last one stops at the iteration that converges
            assert run_calls() - before == -(-sol.iter // spc), (name, s, spc)
    return pieces


def case_idr1_is_bicgstab():
    """shadow = r0 as the single column: the residual norms after every second iteration are BiCGStab's, as long as the
    kappa correction of omega stays out of it - which it does on scaled_system (|rho| >= 0.7 in the first four cycles: the
    two references agree to 6.8e-16 there, and differ by percents on the convection-dominated systems)"""
    A, b = bc.scaled_system()
    want = bicgstab_ref.solve_ref(A, b, TOL, b.size)
    mine = ref.solve_ref(A, b, TOL, 4 * b.size, s=1, shadow=b.reshape(-1, 1))
    between = max(abs(mine.resnorms[2 * j] - want.resnorms[j]) / want.resnorms[j] for j in range(1, 5))
    sol = solve(A, b, s=1, shadow=b.reshape(-1, 1))
    got = max(abs(sol.resnorms[2 * j] - want.resnorms[j]) / want.resnorms[j] for j in range(1, 5))
    print("IDR(1) against BiCGStab: references %.3e, solver %.3e" % (between, got))
    assert between <= RTOL_BICGSTAB / 100
    assert got <= RTOL_BICGSTAB
    assert sol.resnorms[-1] <= TOL


def case_central():
    """a system BiCGStab does not like: IDR(4) converges to 1e-8 within the cap of the whole solves"""
    return case_whole_solve("central32-ones", 4)


def case_initial_guess():
    A, b = system("cd24-ones")
    x0 = np.random.default_rng(7).standard_normal(b.size)
    s0, s1 = solve(A, b), solve(A, b, x0=x0)
    assert s1.resnorms[-1] <= TOL
    assert np.linalg.norm(s1.xk - s0.xk) <= 1e-6 * np.linalg.norm(s0.xk)


def case_shapes():
    A, b = system("cd24-ones")
    flat, col = solve(A, b), solve(A, b.reshape(-1, 1))
    assert flat.linear_system.flat_vecs and not col.linear_system.flat_vecs
    assert flat.xk.shape == (b.size, 1) and col.xk.shape == (b.size, 1)
    assert flat.resnorms == col.resnorms


def case_zero_rhs():
    A, b = system("cd24-ones")
    sol = solve(A, np.zeros(b.size))
    assert sol.resnorms == [0.0] and sol.iter == 0
    assert not np.any(sol.xk)


def case_maxiter():
    from krypy_amd import utils
    A, b = system("cd24-ones")
    with pytest.raises(utils.ConvergenceError) as ei:
        solve(A, b, maxiter=3)
    assert ei.value.solver.iter == 3
    assert len(ei.value.solver.resnorms) == 4


def case_generic(side, s=4):
    """Ml or Mr = the inverse diagonal: a composite operator, so the pieces"""
    A, b = bc.scaled_system()
    D = sp.diags(1.0 / A.diagonal())
    kw = {side: D}
    sol = solve(A, b, s=s, **kw)
    assert sol.resnorms[-1] <= TOL
    want = ref.solve_ref(A, b, TOL, 4 * b.size, s=s, **kw)
    np.testing.assert_allclose(sol.resnorms[1:9], want.resnorms[1:9], rtol=RTOL, atol=0)
    Ml = D if side == "Ml" else sp.identity(b.size)
    x = sol.xk.reshape(-1)
    assert np.linalg.norm(Ml.dot(b - A.dot(x))) / np.linalg.norm(Ml.dot(b)) <= TOL * (1 + 1e-6)
    return sol


def case_refusals():
    from krypy_amd import linsys, utils
    A, b = system("cd24-ones")
    n = b.size
    Id = sp.identity(n, format="csr")
    with pytest.raises(utils.ArgumentError, match="Ml"):
        linsys.Idrs(linsys.LinearSystem(A, b, M=sp.diags(np.full(n, 2.0))))
    with pytest.raises(utils.ArgumentError, match="Ml"):
        linsys.Idrs(linsys.LinearSystem(A, b, Minv=sp.diags(np.full(n, 2.0))))
    with pytest.raises(utils.ArgumentError, match="inner product"):
        linsys.Idrs(linsys.LinearSystem(A, b, ip_B=sp.diags(np.full(n, 2.0))))
    linsys.Idrs(linsys.LinearSystem(A, b, ip_B=None, M=None), tol=TOL)
    with pytest.raises(utils.ArgumentError, match="store_arnoldi"):
        linsys.Idrs(linsys.LinearSystem(A, b), store_arnoldi=True)
    with pytest.raises(NotImplementedError):
        linsys.Idrs(linsys.LinearSystem(A.astype(complex), b))
    with pytest.raises(NotImplementedError):
        linsys.Idrs(linsys.LinearSystem(A, b.astype(complex)))
    with pytest.raises(NotImplementedError):
        linsys.Idrs(linsys.LinearSystem(A, b), x0=np.zeros(n, dtype=complex))
    with pytest.raises(NotImplementedError):
        linsys.Idrs(linsys.LinearSystem(A, b, Ml=Id.astype(complex) * 2))
    with pytest.raises(NotImplementedError):
        linsys.Idrs(linsys.LinearSystem(A, b, Mr=Id.astype(complex) * 2))
    with pytest.raises(utils.ArgumentError):
        linsys.Idrs("not a linear system")
    for s in (0, 9, -1, 2.0):
        with pytest.raises(utils.ArgumentError, match="outside 1"):
            linsys.Idrs(linsys.LinearSystem(A, b), s=s)
    with pytest.raises(utils.ArgumentError, match="shape"):
        linsys.Idrs(linsys.LinearSystem(A, b), s=4, shadow=np.ones((n, 3)))
    with pytest.raises(utils.ArgumentError, match="shape"):
        linsys.Idrs(linsys.LinearSystem(A, b), s=4, shadow=np.ones((n - 1, 4)))
    with pytest.raises(utils.ArgumentError, match="dtype"):
        linsys.Idrs(linsys.LinearSystem(A, b), s=2, shadow=np.ones((n, 2), dtype=complex))
    with pytest.raises(utils.ArgumentError, match="steps_per_call"):
        linsys.Idrs(linsys.LinearSystem(A, b), steps_per_call=65)
    with pytest.raises(utils.ArgumentError, match="steps_per_call"):
        linsys.Idrs(linsys.LinearSystem(A, b), steps_per_call=0)


def case_convenience():
    import krypy_amd
    from krypy_amd import linsys
    A, b = system("cd24-ones")
    for shape in ((b.size,), (b.size, 1)):
        x, sol = krypy_amd.idrs(A, b.reshape(shape), tol=TOL)
        assert isinstance(sol, linsys.Idrs) and sol.s == 4
        assert x.shape == shape and bc.relres(A, x, b) <= TOL * (1 + 1e-6)
    # "not converged" for the wrappers is resnorms[-1] >= tol: A = 2 I ends with a residual of exactly 0, which is not
    # below a tolerance of 0
    x, sol = krypy_amd.idrs(sp.csr_matrix(2.0 * sp.identity(5)), np.arange(1.0, 6.0), s=2, tol=0.0)
    assert x is None and sol.resnorms[-1] == 0.0 and sol.iter == 1
    text = repr(krypy_amd.idrs(A, b, s=2, tol=TOL)[1])
    assert "krypy IDR(s) object" in text and "s: 2" in text
    # s = 4: a cycle of 5 iterations takes 27 inner products and 46 vector updates; the setup 7 and 1
    assert linsys.Idrs.operations(5) == {"A": 6, "M": 2, "Ml": 7, "Mr": 6, "ip_B": 34, "axpy": 47}
    assert linsys.Idrs.operations(3, s=1) == {"A": 4, "M": 2, "Ml": 5, "Mr": 4, "ip_B": 13, "axpy": 12}


# ---- the stop word ----------------------------------------------------------------------------------------------------------
def case_stop_word(ctx):
    """A run of 5 with a tolerance that the second step meets does two steps and leaves P, G, U, r, y exactly as a two-step
    run does (the operator products queued behind the stop write t only); going on from position 2 matches the uninterrupted
    run with tol = 0 step for step."""
    from krypy_amd import _hip
    A, b = system("cd24-ones")
    n, s = b.size, 4
    Amat = ctx.csr(A)
    P0 = np.asfortranarray(np.random.default_rng(2).standard_normal((n, s)))

    def fresh():
        V = ctx.alloc(n, 3)
        V.upload(0, b)
        st = (ctx.upload(P0), 0, ctx.alloc(n, s), 0, ctx.alloc(n, s), 0, V, 0, V, 1, V, 2, ctx.alloc(_hip.IDRS_NSCAL, 1), s)
        assert ctx.idrs_init(st) == float(n)
        return st

    def vectors(st):
        return [st[0].download(), st[2].download(), st[4].download(), st[6].download(0, 2)]

    full = fresh()
    recs = ctx.idrs_run(Amat, full, 0, 7, 1.0, 0.0)
    assert len(recs) == 7 and all(r[3] == 0 for r in recs)
    two = fresh()
    assert ctx.idrs_run(Amat, two, 0, 2, 1.0, 0.0) == recs[:2]
    tol = float(np.sqrt(recs[1][0]))                             # bnorm = 1: met by the second step, not by the first
    assert np.sqrt(recs[0][0]) > tol
    st = fresh()
    assert ctx.idrs_run(Amat, st, 0, 5, 1.0, tol) == recs[:2]    # the counter says 2
    for got, want in zip(vectors(st), vectors(two)):
        assert np.array_equal(got, want)
    sc, sc2 = st[12].download()[:, 0], two[12].download()[:, 0]
    L = _hip.IDRS_LAYOUT
    assert sc[L["STOP"]] == 1.0 and sc[L["COUNT"]] == 2.0 and sc2[L["STOP"]] == 0.0
    for name in ("M", "F", "OM", "RR"):                          # what the iteration goes on from
        width = 64 if name == "M" else 8 if name == "F" else 1
        assert np.array_equal(sc[L[name]: L[name] + width], sc2[L[name]: L[name] + width]), name
    assert ctx.idrs_run(Amat, st, 2, 5, 1.0, 0.0) == recs[2:]
    for got, want in zip(vectors(st), vectors(full)):
        assert np.array_equal(got, want)


# ---- the entry points' own argument checks ------------------------------------------------------------------------------
def case_abi_errors(ctx):
    from krypy_amd import _hip
    n, s = 64, 2
    A = ctx.csr(bc.convdiff(8, 8, 0.5, 0.25))
    B = ctx.alloc(n, 3 * s + 3)
    SC = ctx.alloc(_hip.IDRS_NSCAL, 1)

    def state(**kw):
        d = dict(P=B, pcol=0, G=B, gcol=s, U=B, ucol=2 * s, R=B, rcol=3 * s, YK=B, ycol=3 * s + 1, T=B, tcol=3 * s + 2,
                 SC=SC, s=s)
        d.update(kw)
        return tuple(d[k] for k in ("P", "pcol", "G", "gcol", "U", "ucol", "R", "rcol", "YK", "ycol", "T", "tcol", "SC", "s"))

    ctx.idrs_init(state())                                                   # the good state passes
    BE = _hip.BackendError
    with pytest.raises(BE, match="r and yk share a column"):
        ctx.idrs_run(A, state(ycol=3 * s), 0, 1, 1.0, 0.0)
    with pytest.raises(BE, match="G and U share a column"):                  # overlapping column ranges
        ctx.idrs_run(A, state(ucol=s + 1), 0, 1, 1.0, 0.0)
    with pytest.raises(BE, match="P and t share a column"):
        ctx.idrs_orth(state(tcol=1), 0, 1.0, 0.0)
    with pytest.raises(BE, match="length mismatch \\(t\\)"):
        ctx.idrs_run(A, state(T=ctx.alloc(n - 1, 1), tcol=0), 0, 1, 1.0, 0.0)
    with pytest.raises(BE, match="out of range"):                            # a short block: U has s - 1 columns left
        ctx.idrs_dir(state(U=ctx.alloc(n, s), ucol=1), 0)
    with pytest.raises(BE, match="scalar block is short"):
        ctx.idrs_init(state(SC=ctx.alloc(_hip.IDRS_NSCAL - 1, 1)))
    with pytest.raises(BE, match="real operator"):
        ctx.idrs_run(ctx.csr(bc.convdiff(8, 8, 0.5, 0.25).astype(complex)), state(), 0, 1, 1.0, 0.0)
    with pytest.raises(BE, match="length mismatch \\(operator\\)"):
        ctx.idrs_run(ctx.csr(bc.convdiff(8, 7, 0.5, 0.25)), state(), 0, 1, 1.0, 0.0)
    for bad in (0, 9):
        with pytest.raises(BE, match="s = %d is outside 1 .. 8" % bad):
            ctx.idrs_run(A, state(s=bad), 0, 1, 1.0, 0.0)
    with pytest.raises(BE, match="position 3 is outside 0 .. s = 2"):
        ctx.idrs_run(A, state(), s + 1, 1, 1.0, 0.0)
    with pytest.raises(BE, match="nsteps = 65 is outside 1 .. 64"):
        ctx.idrs_run(A, state(), 0, 65, 1.0, 0.0)
    with pytest.raises(BE, match="nsteps = 0 is outside"):
        ctx.idrs_run(A, state(), 0, 0, 1.0, 0.0)
    with pytest.raises(BE, match="position k = 2 is outside"):
        ctx.idrs_dir(state(), s)
    with pytest.raises(BE, match="position k = 2 is outside"):
        ctx.idrs_orth(state(), s, 1.0, 0.0)
    with pytest.raises(BE):
        ctx.idrs_init(state(R=ctx.alloc(n, 1, dtype=np.complex128), rcol=0))
