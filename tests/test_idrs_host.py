"""CPU tests of IDR(s): the NumPy reference against itself (four summation orders) and against BiCGStab's, and the host layer
(``linsys.Idrs``, ``krypy_amd.idrs``) on a NumPy context whose ``idrs_*`` entries are that reference."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import bicgstab_cases as bc
from tests.support import idrs_cases as ic
from tests.support import idrs_ref as ref


@pytest.fixture
def idrs_double():
    from krypy_amd import _hip
    from tests.support.idrs_numpy_context import IdrsNumpyContext

    ctx = IdrsNumpyContext()
    old = _hip._install_context_for_testing(ctx)
    yield ctx
    _hip._install_context_for_testing(old)


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_central_is_the_definition():
    A = ic.central(4, 3, 0.5, 0.25).toarray()
    assert A.shape == (12, 12)
    assert A[5, 5] == 4.0
    assert A[5, 4] == -1.5 and A[5, 6] == -0.5 and A[5, 1] == -1.25 and A[5, 9] == -0.75
    assert A[4, 3] == 0.0 and A[3, 4] == 0.0                    # no coupling across the end of a grid row


def test_shadow_is_orthonormal_and_repeatable():
    from krypy_amd import utils
    P = utils.idrs_shadow(50, 4, seed=3)
    assert P.shape == (50, 4) and P.dtype == np.float64
    assert np.allclose(P.T.dot(P), np.eye(4), atol=1e-14)
    assert np.array_equal(P, utils.idrs_shadow(50, 4, seed=3)) and not np.array_equal(P, utils.idrs_shadow(50, 4, seed=4))
    with pytest.raises(utils.ArgumentError):
        utils.idrs_shadow(3, 4)


@pytest.mark.parametrize("name,s", ic.WHOLE)
def test_reference_orders_agree(name, s):
    """The four summation orders of the reference: resnorms[1:9] to 2e-11 (a hundredth of the solver tests' bound), every
    run converged, and the 15 % cap of the solver tests holds among the orders themselves."""
    refs = ic.reference(name, s)
    A, b = ic.system(name)
    counts = sorted(r.iter for r in refs.values())
    spread = ic.order_spread(name, s)
    print("%s s = %d: spread of resnorms[1:9] %.2e, iterations %s" % (name, s, spread, counts))
    assert spread <= ic.RTOL / 100
    for r in refs.values():
        assert r.breakdown is None and r.resnorms[-1] <= ic.TOL
        assert bc.relres(A, r.x, b) <= 1e-7
    assert counts[-1] <= 1.15 * counts[0]


def test_reference_counts_of_the_prototype():
    """the operator applications the issue's prototype needed (identical across the orders on the convdiff systems)"""
    for name, s, want in (("cd24-ones", 4, 97), ("cd37x23-rng", 4, 94), ("cd40-ones", 4, 99), ("cd24-ones", 8, 91)):
        assert {r.iter for r in ic.reference(name, s).values()} == {want}
    assert 141 <= min(r.iter for r in ic.reference("central32-ones", 4).values())
    assert max(r.iter for r in ic.reference("central32-ones", 4).values()) <= 143


def test_forward_substitutions_solve_their_systems():
    """csolve and asolve against numpy.linalg.solve on a random lower-triangular M"""
    rng = np.random.default_rng(5)
    s = 6
    sc = ref.new_scalars()
    Mfull = np.tril(rng.standard_normal((s, s))) + 3 * np.eye(s)
    for i in range(s):
        sc[ref.L["M"] + i * ref.SM: ref.L["M"] + i * ref.SM + s] = Mfull[i]
    f, h = rng.standard_normal(s), rng.standard_normal(s)
    sc[ref.L["F"]: ref.L["F"] + s], sc[ref.L["H"]: ref.L["H"] + s] = f, h
    for k in range(s):
        c, flags = ref.csolve(sc, k, s)
        assert flags == 0 and np.allclose(c[k:], np.linalg.solve(Mfull[k:, k:], f[k:]), rtol=1e-12)
        a, col, beta, fnew, flags = ref.asolve(sc, k, s)
        assert flags == 0
        if k:
            assert np.allclose(a, np.linalg.solve(Mfull[:k, :k], h[:k]), rtol=1e-12)
        assert np.allclose(col, h[k:] - Mfull[k:, :k].dot(a), rtol=1e-12, atol=1e-14)
        assert beta == f[k] / col[0] and np.allclose(fnew, f[k + 1:] - beta * np.array(col[1:]), rtol=1e-12, atol=1e-14)


def test_flags_of_the_reference():
    sc = ref.new_scalars()
    sc[ref.L["M"]] = 0.0
    assert ref.flags_of("dir", sc, 0, 2) == ref.PIVOT_ZERO
    sc[ref.L["H"]] = 0.0
    assert ref.flags_of("orth", sc, 0, 2) == ref.PIVOT_ZERO
    sc[ref.L["H"] + 1] = np.inf
    assert ref.flags_of("orth", sc, 0, 2) == ref.PIVOT_ZERO | ref.NONFINITE
    assert ref.omega_scalars(0.0, 0.0, 1.0) == (0.0, ref.OMEGA_CLAMPED | ref.OMEGA_ZERO)
    assert ref.omega_scalars(0.0, 2.0, 1.0) == (0.0, ref.OMEGA_ZERO)
    assert ref.omega_scalars(np.nan, 2.0, 1.0) == (0.0, ref.NONFINITE | ref.OMEGA_ZERO)
    om, flags = ref.omega_scalars(1.0, 2.0, 1.0)                 # rho = 1 / sqrt(2) >= 0.7: no correction
    assert (om, flags) == (0.5, 0)
    om, flags = ref.omega_scalars(1.0, 4.0, 1.0)                 # rho = 0.5 < 0.7: om = (0.25 * 0.7) / 0.5
    assert (om, flags) == ((0.25 * 0.7) / 0.5, 0)


# ---- the host layer on the double ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 3, 5])
def test_multiple_of_identity(idrs_double, s):
    ic.case_multiple_of_identity(s)


def test_swap_breakdown(idrs_double):
    ic.case_swap_breakdown()


@pytest.mark.parametrize("name,s", ic.WHOLE)
def test_whole_solve(idrs_double, name, s):
    sol = ic.case_whole_solve(name, s)
    # a plain matrix: runs of s + 1 iterations, none of the pieces
    c = idrs_double.calls
    assert c["idrs_run"] == -(-sol.iter // (s + 1)) and c["idrs_init"] == 1
    assert not any(k in c for k in ("idrs_dir", "idrs_orth", "idrs_omega", "apply"))
    assert idrs_double.get("n_idrs_steps") == sol.iter


def test_double_and_reference_are_the_same_bits(idrs_double):
    """numpy.dot in both: the solver on the double reproduces solve_ref's trace exactly"""
    A, b = ic.system("cd37x23-rng")
    sol = ic.solve(A, b, s=4)
    want = ref.solve_ref(A, b, ic.TOL, 4 * b.size, s=4)
    assert list(sol.idrs_trace) == want.trace[-len(sol.idrs_trace):] and len(sol.idrs_trace) == 16
    assert sol.iter == want.iter


@pytest.mark.parametrize("name,s", ic.PAIRS)
def test_run_against_pieces(idrs_double, name, s):
    ic.case_run_against_pieces(name, s, lambda: idrs_double.calls.get("idrs_run", 0))


def test_host_callable_operator(idrs_double):
    """an operator that is a host callable takes the pieces and computes the same sequence as the runs"""
    from krypy_amd import utils
    A, b = ic.system("cd24-ones")
    op = utils.LinearOperator(A.shape, float, dot=lambda X: A.dot(X))
    s_op, s_mat = ic.solve(op, b), ic.solve(A, b)
    assert s_op.resnorms == s_mat.resnorms and np.array_equal(s_op.xk, s_mat.xk)
    assert idrs_double.calls["idrs_orth"] + idrs_double.calls["idrs_omega"] == s_op.iter


def test_stop_word(idrs_double):
    ic.case_stop_word(idrs_double)


def test_initial_guess(idrs_double):
    ic.case_initial_guess()


def test_shapes(idrs_double):
    ic.case_shapes()


def test_zero_rhs(idrs_double):
    ic.case_zero_rhs()
    assert not any(k.startswith("idrs") for k in idrs_double.calls)


def test_maxiter(idrs_double):
    ic.case_maxiter()
    # two iterations in one run, the last one - whose iterate the explicit residual needs - by the pieces
    c = idrs_double.calls
    assert c["idrs_run"] == 1 and c["idrs_dir"] == 1 and c["idrs_orth"] == 1


@pytest.mark.parametrize("side", ["Ml", "Mr"])
def test_generic_path(idrs_double, side):
    sol = ic.case_generic(side)
    c = idrs_double.calls
    assert "idrs_run" not in c
    assert c["idrs_dir"] == c["idrs_orth"] and c["idrs_orth"] + c["idrs_omega"] == sol.iter


def test_idr1_is_bicgstab(idrs_double):
    ic.case_idr1_is_bicgstab()


def test_central(idrs_double):
    ic.case_central()


def test_explicit_residual_and_errnorms(idrs_double):
    from krypy_amd import linsys
    A, b = ic.system("cd24-ones")
    x = np.linalg.solve(A.toarray(), b)
    sol = linsys.Idrs(linsys.LinearSystem(A, b, exact_solution=x), tol=ic.TOL, explicit_residual=True)
    assert sol.resnorms[-1] <= ic.TOL and len(sol.errnorms) == len(sol.resnorms)
    assert sol.errnorms[-1] <= 1e-6 * np.linalg.norm(x)
    assert "idrs_run" not in idrs_double.calls                   # every iterate is wanted: the pieces


def test_explicit_shadow(idrs_double):
    from krypy_amd import utils
    A, b = ic.system("cd24-ones")
    P = utils.idrs_shadow(b.size, 4, seed=0)
    assert ic.solve(A, b, shadow=P).resnorms == ic.solve(A, b).resnorms
    Pd = idrs_double.upload(P)                                   # a device block is taken as it is, and left as it is
    assert ic.solve(A, b, shadow=Pd).resnorms == ic.solve(A, b).resnorms and np.array_equal(Pd.download(), P)
    with pytest.raises(utils.ArgumentError, match="shape"):
        ic.solve(A, b, s=3, shadow=Pd)
    assert ic.solve(A, b, seed=1).resnorms != ic.solve(A, b).resnorms


def test_refusals(idrs_double):
    ic.case_refusals()


def test_convenience(idrs_double):
    ic.case_convenience()


def test_abi_errors_of_the_double(idrs_double):
    ic.case_abi_errors(idrs_double)
