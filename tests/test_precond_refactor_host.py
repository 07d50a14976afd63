"""Characterisation of the device preconditioners' Python layer (krypy_amd/precond.py) on the NumPy test double: every argument
error's type and message, and for the two persistent classes (``Ilu0Preconditioner``, ``BlockJacobiPreconditioner``) the double's
call counts and the ``info`` property after each step of a scripted life.  The expected values are
tests/golden/precond_messages.json, recorded from the commit named in the file, the last one that had these classes inside
``utils.py``, by ``python -m tests.test_precond_refactor_host`` there (everything is reached through the ``utils`` spellings, which
both layouts have).  The file is a record of that commit: a value that has to be edited means the behaviour has changed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "precond_messages.json")

MOVED = ["TriangularSolveOperator", "ilu_operator", "Ilu0Factors", "ilu0", "ilu0_operator", "Ilu0Preconditioner",
         "ilu0_preconditioner", "spai", "spai_operator", "fsai", "fsai_operator", "block_jacobi", "BlockJacobiPreconditioner",
         "block_jacobi_operator", "chebyshev_coefficients", "ChebyshevOperator", "chebyshev_operator"]


def _double():
    from tests.support.bjac_numpy_context import BjacNumpyContext
    from tests.support.cheb_numpy_context import ChebNumpyContext
    from tests.support.fsai_numpy_context import FsaiNumpyContext
    from tests.support.ilu0p_numpy_context import Ilu0pNumpyContext
    from tests.support.spai_numpy_context import SpaiNumpyContext

    class Double(Ilu0pNumpyContext, BjacNumpyContext, SpaiNumpyContext, FsaiNumpyContext, ChebNumpyContext):
        """Every preconditioner entry of the doubles in one context (each class only adds methods to NumpyContext)."""

    return Double()


def _plain(x):
    """``x`` as JSON gives it back: NumPy scalars become Python's, tuples lists."""
    def default(o):
        if isinstance(o, np.generic):
            return o.item()
        raise TypeError(type(o))
    return json.loads(json.dumps(x, default=default))


def _error(name, fn):
    try:
        fn()
    except Exception as e:       # noqa: BLE001  (the type is what gets recorded)
        return [type(e).__name__, str(e)]
    raise AssertionError("no error raised: " + name)


def _tridiag(n, cplx=False):
    A = sp.diags([-np.ones(n - 1), 2.0 + 0.25 * np.arange(n), -0.5 * np.ones(n - 1)], [-1, 0, 1]).tocsr()
    return (A + 0.5j * sp.identity(n)).tocsr() if cplx else A


def _stored_zero(A, i, j):
    """``A`` with the stored entry (i, j) set to 0 (it stays in the pattern)."""
    A = A.copy()
    k = A.indptr[i] + int(np.flatnonzero(A.indices[A.indptr[i]:A.indptr[i + 1]] == j)[0])
    A.data[k] = 0.0
    return A


def _without(A, i, j):
    """``A`` without the entry (i, j) in its pattern."""
    L = A.tolil()
    L[i, j] = 0
    A = sp.csr_matrix(L)
    A.eliminate_zeros()
    return A


def _message_cases(utils, ctx):
    """``[(name, thunk)]``: every thunk raises."""
    A = _tridiag(6)
    Ac = _tridiag(6, True)
    rect = sp.csr_matrix(np.ones((4, 5)))
    vec, cube = np.ones(3), np.ones((2, 2, 2))
    dev = utils.DeviceOperator(ctx.csr(A))
    nodiag = _without(A, 2, 2)
    piv0 = _stored_zero(A, 0, 0)                                  # ILU(0): pivot 0 is zero
    big = sp.identity(40, format="csr")
    full = np.ones((40, 40))
    sing = A.copy().tolil()
    sing[2, :] = 0
    sing[3, :] = 0
    sing = sp.csr_matrix(sing)
    sing.eliminate_zeros()                                        # block-Jacobi: block 1 of size 2 is zero
    nonherm = _tridiag(6)                                         # (its two off-diagonals differ)
    lowerT = sp.tril(A).tocsr()
    C = []

    def case(name, fn):
        C.append((name, fn))

    persistent = {"Ilu0Preconditioner": utils.Ilu0Preconditioner, "ilu0_preconditioner": utils.ilu0_preconditioner}
    builders = dict(ilu0=utils.ilu0, ilu0_operator=utils.ilu0_operator, spai=utils.spai, spai_operator=utils.spai_operator,
                    fsai=utils.fsai, fsai_operator=utils.fsai_operator,
                    block_jacobi=lambda M: utils.block_jacobi(M, block_size=2),
                    BlockJacobiPreconditioner=lambda M: utils.BlockJacobiPreconditioner(M, block_size=2),
                    block_jacobi_operator=lambda M: utils.block_jacobi_operator(M, block_size=2),
                    block_jacobi_operator_matrix=lambda M: utils.block_jacobi_operator(M, block_size=2, form="matrix"),
                    TriangularSolveOperator=utils.TriangularSolveOperator,
                    ChebyshevOperator=lambda M: utils.ChebyshevOperator(M, 4.0),
                    chebyshev_operator=utils.chebyshev_operator, **persistent)
    for name, fn in sorted(builders.items()):
        case("not 2-D, 1-D: " + name, lambda fn=fn: fn(vec))
        case("not 2-D, 3-D: " + name, lambda fn=fn: fn(cube))
        case("not square: " + name, lambda fn=fn: fn(rect))
        case("not square, dense float32: " + name, lambda fn=fn: fn(np.ones((4, 5), dtype=np.float32)))
        if "hebyshev" not in name:               # (a Chebyshev operator takes a device-only operator)
            case("device-only operator: " + name, lambda fn=fn: fn(dev))
    case("device-only operator: ChebyshevOperator scale='jacobi'", lambda: utils.ChebyshevOperator(dev, 4.0, scale="jacobi"))
    case("device-only operator: spai pattern", lambda: utils.spai(A, pattern=dev))
    case("device-only operator: fsai pattern", lambda: utils.fsai(A, pattern=dev))
    case("not square: TriangularSolveOperator of a MatrixLinearOperator",
         lambda: utils.TriangularSolveOperator(utils.MatrixLinearOperator(lowerT)))

    for name in ("ilu0", "ilu0_operator", "Ilu0Preconditioner", "ilu0_preconditioner"):
        fn = getattr(utils, name)
        case("unknown ordering: " + name, lambda fn=fn: fn(A, ordering="rcm"))
        case("unknown ordering comes before the matrix: " + name, lambda fn=fn: fn(vec, ordering="rcm"))
        case("missing diagonal: " + name, lambda fn=fn: fn(nodiag))
        case("missing diagonal, multicolor: " + name, lambda fn=fn: fn(nodiag, "multicolor"))
        case("broken pivot: " + name, lambda fn=fn: fn(piv0))
        case("broken pivot, multicolor: " + name, lambda fn=fn: fn(_stored_zero(A, 2, 2), "multicolor"))
        case("broken pivot, complex: " + name, lambda fn=fn: fn(_stored_zero(Ac, 0, 0)))
    case("unknown side: spai", lambda: utils.spai(A, side="both"))
    case("unknown side comes before the matrix: spai", lambda: utils.spai(vec, side="both"))
    case("unknown side: spai_operator", lambda: utils.spai_operator(A, side="both"))
    case("unknown form: fsai_operator", lambda: utils.fsai_operator(A, form="dense"))
    case("unknown form: block_jacobi_operator", lambda: utils.block_jacobi_operator(A, block_size=2, form="dense"))

    for name, fn in (("spai", utils.spai), ("fsai", utils.fsai), ("spai_operator", utils.spai_operator),
                     ("fsai_operator", utils.fsai_operator)):
        Ah = (A + A.T).tocsr()
        case("pattern of the wrong shape, sparse: " + name, lambda fn=fn: fn(Ah, pattern=sp.identity(5, format="csr")))
        case("pattern of the wrong shape, dense: " + name, lambda fn=fn: fn(Ah, pattern=np.ones((6, 7))))
        case("pattern of the wrong shape, operator: " + name,
             lambda fn=fn: fn(Ah, pattern=utils.MatrixLinearOperator(sp.identity(5, format="csr"))))
        case("pattern not 2-D: " + name, lambda fn=fn: fn(Ah, pattern=vec))
        case("pattern row of 33 entries: " + name, lambda fn=fn: fn(big, pattern=full))
    P33 = sp.lil_matrix((40, 40))
    P33[5, :33] = 1
    P33 = (sp.csr_matrix(P33) + sp.identity(40)).tocsr()
    case("pattern row of 33 entries, row 5: spai", lambda: utils.spai(big, pattern=P33))
    case("pattern column of 33 entries, column 5: spai", lambda: utils.spai(big, pattern=P33.T.tocsr(), side="right"))
    case("pattern row of 33 entries in the lower triangle: fsai", lambda: utils.fsai(big, pattern=sp.tril(full).tocsr()))
    case("not Hermitian: fsai", lambda: utils.fsai(nonherm))
    case("not Hermitian: fsai_operator", lambda: utils.fsai_operator(nonherm))
    case("not Hermitian, complex: fsai", lambda: utils.fsai((Ac + Ac.T).tocsr()))
    case("not positive definite: fsai", lambda: utils.fsai((-sp.identity(5)).tocsr()))
    case("dependent rows: spai", lambda: utils.spai(np.ones((4, 4))))
    case("dependent rows: spai right", lambda: utils.spai(np.ones((4, 4)), side="right"))

    n = A.shape[0]
    bjacs = (("block_jacobi", utils.block_jacobi), ("BlockJacobiPreconditioner", utils.BlockJacobiPreconditioner),
             ("block_jacobi_operator", utils.block_jacobi_operator))
    for name, fn in bjacs:
        for what, kw in (("neither", dict()), ("both", dict(block_size=2, blocks=[0, n])), ("block_size 0", dict(block_size=0)),
                         ("block_size 33", dict(block_size=33)), ("block_size 2.0", dict(block_size=2.0)),
                         ("block_size True", dict(block_size=True)), ("blocks wrong start", dict(blocks=[1, n])),
                         ("blocks wrong end", dict(blocks=[0, n - 1])), ("blocks not increasing", dict(blocks=[0, 4, 4, n])),
                         ("blocks decreasing", dict(blocks=[0, 5, 4, n])), ("blocks of floats", dict(blocks=[0.0, float(n)])),
                         ("blocks of one entry", dict(blocks=[0])), ("blocks 2-D", dict(blocks=[[0, n]]))):
            case("bad partition, %s: %s" % (what, name), lambda fn=fn, kw=kw: fn(A, **kw))
        case("bad partition, a block of 33 rows: " + name, lambda fn=fn: fn(big, blocks=[0, 3, 36, 40]))
        case("bad partition comes after the matrix: " + name, lambda fn=fn: fn(rect, block_size=0))
        case("broken block: " + name, lambda fn=fn: fn(sing, block_size=2))
        case("broken block, blocks: " + name, lambda fn=fn: fn(sing, blocks=[0, 1, 4, 6]))

    # update() of the two persistent classes, and what follows a failed one
    for name, make, broken in (("Ilu0Preconditioner", lambda M: utils.Ilu0Preconditioner(M), piv0),
                               ("Ilu0Preconditioner multicolor", lambda M: utils.Ilu0Preconditioner(M, "multicolor"),
                                _stored_zero(A, 2, 2)),
                               ("BlockJacobiPreconditioner", lambda M: utils.BlockJacobiPreconditioner(M, block_size=2), sing)):
        bj = name.startswith("Block")
        ok = sp.csr_matrix(sp.block_diag([np.ones((2, 2)) + np.eye(2)] * 3)) if bj else A
        M = make(ok)
        if bj:                  # the broken update keeps the pattern: zeros stored in block 1
            broken = ok.copy()
            broken.data[broken.indptr[2]:broken.indptr[4]] = 0.0
        case("update, wrong shape: " + name, lambda M=M: M.update(_tridiag(5)))
        case("update, wrong dtype: " + name, lambda M=M, ok=ok: M.update(ok.astype(np.complex128)))
        case("update, float32 is widened, then the pattern: " + name,
             lambda M=M, ok=ok: M.update(_without(ok, 1, 0).astype(np.float32)))
        case("update, pattern with fewer entries in row 1: " + name, lambda M=M, ok=ok: M.update(_without(ok, 1, 0)))
        moved = ok.copy().tolil()          # as many entries in every row: the row pointers agree, the columns do not
        moved[4, 5] = 0
        moved[4, 0] = 1.0
        moved = sp.csr_matrix(moved)
        moved.eliminate_zeros()
        case("update, pattern with another column in row 4: " + name, lambda M=M, moved=moved: M.update(moved))
        extra = sp.csr_matrix(ok + sp.csr_matrix(([1.0], ([n - 1], [0])), shape=ok.shape))
        case("update, pattern with one more entry in the last row: " + name, lambda M=M, extra=extra: M.update(extra))
        case("update, not 2-D: " + name, lambda M=M: M.update(vec))
        case("update, not square: " + name, lambda M=M: M.update(rect))
        case("update, device-only operator: " + name, lambda M=M: M.update(dev))
        if not bj:
            case("update, missing diagonal: " + name, lambda M=M: M.update(nodiag))
        case("update, breakdown: " + name, lambda M=M, broken=broken: M.update(broken))
        x = np.ones((n, 2))
        case("after a failed update, dot: " + name, lambda M=M: M.dot(x))
        case("after a failed update, on device blocks: " + name,
             lambda M=M: M._apply_dev(ctx.upload(x), 0, ctx.alloc(n, 2), 0, 2))
        case("after a failed update, dot_adj: " + name, lambda M=M: M.dot_adj(x))
        if bj:
            case("after a failed update, matrix(): " + name, lambda M=M: M.matrix())

    # a complex operator on a real device block
    Xr, Yr = ctx.alloc(n, 1), ctx.alloc(n, 1)
    Cl = sp.tril(Ac).tocsr()
    for name, make in (("MatrixLinearOperator", lambda: utils.MatrixLinearOperator(Ac)),
                       ("MatrixLinearOperator dense", lambda: utils.MatrixLinearOperator(Ac.toarray())),
                       ("TriangularSolveOperator", lambda: utils.TriangularSolveOperator(Cl)),
                       ("Ilu0Preconditioner", lambda: utils.Ilu0Preconditioner(Ac)),
                       ("BlockJacobiPreconditioner", lambda: utils.BlockJacobiPreconditioner(Ac, block_size=3)),
                       ("ChebyshevOperator", lambda: utils.ChebyshevOperator(Ac, 4.0)),
                       ("ChebyshevOperator of an operator", lambda: utils.ChebyshevOperator(
                           utils.LinearOperator((n, n), complex, dot=lambda X: X), 4.0))):
        case("complex on a real device block: " + name, lambda make=make: make()._apply_dev(Xr, 0, Yr, 0, 1))

    T = utils.TriangularSolveOperator
    case("TriangularSolveOperator: not triangular", lambda: T(A))
    case("TriangularSolveOperator: lower=True with entries above", lambda: T(sp.triu(A).tocsr(), lower=True))
    case("TriangularSolveOperator: lower=False with entries below", lambda: T(lowerT, lower=False))
    case("TriangularSolveOperator: lower=True for a full matrix", lambda: T(A, lower=True))
    case("TriangularSolveOperator: missing diagonal", lambda: T(_without(lowerT, 3, 3)))
    case("TriangularSolveOperator: zero diagonal", lambda: T(_stored_zero(lowerT, 2, 2), lower=True))
    case("TriangularSolveOperator: dense, not triangular", lambda: T(A.toarray().astype(np.float32)))
    case("ilu_operator: a factor that is not triangular",
         lambda: utils.ilu_operator(type("F", (), dict(L=A, U=A, perm_r=np.arange(n), perm_c=np.arange(n)))()))

    Ch = utils.ChebyshevOperator
    S = (A + A.T).tocsr()
    case("ChebyshevOperator: lmin above lmax", lambda: Ch(S, 1.0, lmin=2.0))
    case("ChebyshevOperator: lmin equal to lmax", lambda: Ch(S, 1.0, lmin=1.0))
    case("ChebyshevOperator: negative lmax", lambda: Ch(S, -1.0))
    case("ChebyshevOperator: lmin zero", lambda: Ch(S, 4.0, lmin=0.0))
    case("ChebyshevOperator: infinite lmax", lambda: Ch(S, float("inf"), lmin=1.0))
    case("ChebyshevOperator: nan lmax", lambda: Ch(S, float("nan")))
    case("ChebyshevOperator: degree 0", lambda: Ch(S, 4.0, degree=0))
    case("ChebyshevOperator: degree 1.5", lambda: Ch(S, 4.0, degree=1.5))
    case("ChebyshevOperator: degree None", lambda: Ch(S, 4.0, degree=None))
    case("ChebyshevOperator: degree comes before the bounds", lambda: Ch(S, -1.0, degree=0))
    case("ChebyshevOperator: unknown scale", lambda: Ch(S, 4.0, scale="ruiz"))
    case("ChebyshevOperator: scale='jacobi' of a callable",
         lambda: Ch(utils.LinearOperator((n, n), float, dot=lambda X: X), 4.0, scale="jacobi"))
    case("ChebyshevOperator: scale of the wrong length", lambda: Ch(S, 4.0, scale=np.ones(n + 1)))
    case("ChebyshevOperator: scale 2-D", lambda: Ch(S, 4.0, scale=np.ones((n, 1))))
    case("ChebyshevOperator: scale with a complex entry", lambda: Ch(S, 4.0, scale=np.ones(n) + 1j))
    case("ChebyshevOperator: scale with a zero", lambda: Ch(S, 4.0, scale=np.arange(n, dtype=float)))
    case("ChebyshevOperator: scale with an infinity", lambda: Ch(S, 4.0, scale=np.full(n, np.inf)))
    case("ChebyshevOperator: scale='jacobi' with a negative diagonal", lambda: Ch(-S, 4.0, scale="jacobi"))
    case("ChebyshevOperator: not square operator", lambda: Ch(utils.MatrixLinearOperator(rect), 4.0))
    case("chebyshev_operator: degree 0", lambda: utils.chebyshev_operator(S, degree=0))
    case("chebyshev_operator: unknown scale", lambda: utils.chebyshev_operator(S, scale="ruiz"))
    return C


def _life(utils, ctx, make, good, broken, cplx_first=False):
    """The scripted life of a persistent preconditioner: after every step the double's call counts and ``info``."""
    n = good.shape[0]
    rng = np.random.RandomState(11)
    xr = rng.randn(n, 2)
    xc = xr + 1j * rng.randn(n, 2)
    other = good.copy()
    other.data = other.data * rng.uniform(0.75, 1.25, other.nnz)
    M = [None]
    out = []

    def step(name, fn):
        rec = dict(step=name)
        try:
            got = fn()
            if isinstance(got, np.ndarray):
                rec["result"] = dict(dtype=str(got.dtype), shape=list(got.shape), contiguous=bool(got.flags.c_contiguous))
        except Exception as e:       # noqa: BLE001
            rec["error"] = [type(e).__name__, str(e)]
        rec["calls"] = dict(ctx.calls)
        rec["info"] = None if M[0] is None else M[0].info
        rec["repr"] = repr(M[0])
        out.append(_plain(rec))

    def construct():
        M[0] = make(good)

    step("construct", construct)
    step("apply to a real block", lambda: M[0].dot(xr))
    step("apply to a complex block", lambda: M[0].dot(xc))
    step("apply on the device, one column of a real block", lambda: M[0]._apply_dev(ctx.upload(xr), 1, ctx.alloc(n, 3), 2, 1))
    step("times a device vector", lambda: (M[0] * utils.DVec.from_host(xr[:, :1])).download())
    step("update", lambda: M[0].update(other))
    step("apply after the update", lambda: M[0].dot(xr))
    step("failed update", lambda: M[0].update(broken))
    step("apply after the failed update", lambda: M[0].dot(xr))
    step("refused update (another shape) after the failed one", lambda: M[0].update(good[:n - 1][:, :n - 1].tocsr()))
    step("successful update", lambda: M[0].update(good))
    step("apply after the successful update", lambda: M[0].dot(xc))
    return out


def record():
    """Everything the fixture holds, from the code as it stands."""
    from krypy_amd import _hip, utils

    out = dict(utils_all=list(utils.__all__), messages={}, scenarios={})
    ctx = _double()
    old = _hip._install_context_for_testing(ctx)
    try:
        for name, fn in _message_cases(utils, ctx):
            assert name not in out["messages"], name
            out["messages"][name] = _error(name, fn)
    finally:
        _hip._install_context_for_testing(old)

    A = _tridiag(7)
    A = (A + sp.csr_matrix(([0.5, -0.25], ([0, 5], [4, 1])), shape=A.shape)).tocsr()
    B = sp.csr_matrix(sp.block_diag([np.array([[4.0, 1, 0], [1, 3, 1], [0.5, 1, 5]])] * 2 + [np.array([[2.0]])])
                      + sp.csr_matrix(([0.5], ([0], [6])), shape=(7, 7)))
    B.sort_indices()
    Bbad = B.copy()
    Bbad.data[Bbad.indptr[3]:Bbad.indptr[6]] = 0.0
    lives = {
        "Ilu0Preconditioner natural": (lambda M: utils.Ilu0Preconditioner(M), A, _stored_zero(A, 0, 0)),
        "Ilu0Preconditioner multicolor": (lambda M: utils.ilu0_preconditioner(M, "multicolor"), A, _stored_zero(A, 2, 2)),
        "Ilu0Preconditioner complex": (lambda M: utils.Ilu0Preconditioner(M), (A + 0.5j * sp.identity(7)).tocsr(),
                                       _stored_zero((A + 0.5j * sp.identity(7)).tocsr(), 0, 0)),
        "BlockJacobiPreconditioner block_size": (lambda M: utils.BlockJacobiPreconditioner(M, block_size=3), B, Bbad),
        "BlockJacobiPreconditioner blocks": (lambda M: utils.block_jacobi_operator(M, blocks=[0, 3, 6, 7]), B, Bbad),
        "BlockJacobiPreconditioner float32": (lambda M: utils.BlockJacobiPreconditioner(M, block_size=3), B.astype(np.float32),
                                              Bbad.astype(np.float32)),
    }
    for name, (make, good, broken) in lives.items():
        ctx = _double()
        old = _hip._install_context_for_testing(ctx)
        try:
            out["scenarios"][name] = _life(utils, ctx, make, good, broken)
        finally:
            _hip._install_context_for_testing(old)
    return _plain(out)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    return record()


def test_every_message_is_the_recorded_one(recorded, replayed):
    assert sorted(replayed["messages"]) == sorted(recorded["messages"])
    for name, want in recorded["messages"].items():
        assert replayed["messages"][name] == want, name


def test_the_persistent_classes_make_the_recorded_calls(recorded, replayed):
    assert sorted(replayed["scenarios"]) == sorted(recorded["scenarios"])
    for name, steps in recorded["scenarios"].items():
        got = replayed["scenarios"][name]
        assert [s["step"] for s in got] == [s["step"] for s in steps], name
        for g, w in zip(got, steps):
            assert g == w, (name, w["step"])


def test_the_fixture_covers_what_it_is_for(recorded):
    """Guards the recording itself: both kinds of outcome occur in every life, and the second handle appears."""
    for name, steps in recorded["scenarios"].items():
        by = {s["step"]: s for s in steps}
        assert "error" not in by["construct"] and "error" not in by["successful update"], name
        assert by["failed update"]["error"][0] == "ArgumentError", name
        assert by["apply after the failed update"]["error"][0] == "LinearOperatorError", name
        create = "ilu0_handle" if name.startswith("Ilu0") else "bjac_create"
        second = 1 if "complex" in name else 2
        assert by["construct"]["calls"][create] == 1 and by["apply to a complex block"]["calls"][create] == second, name
    assert len(recorded["messages"]) > 200
    assert sum(1 for t, m in recorded["messages"].values() if "applied to a real device block" in m) == 7


def test_utils_reexports_the_objects_of_precond(recorded):
    from krypy_amd import precond, utils

    assert list(utils.__all__) == recorded["utils_all"]
    assert sorted(precond.__all__) == sorted(MOVED)
    for name in MOVED:
        assert getattr(utils, name) is getattr(precond, name), name
        assert getattr(precond, name).__module__ == "krypy_amd.precond", name


@pytest.mark.parametrize("first", ["import krypy_amd.precond", "from krypy_amd.precond import ChebyshevOperator"])
def test_precond_can_be_the_first_import_of_the_package(first):
    """In a fresh interpreter; no GPU and no library load are needed to import."""
    code = first + "; import sys; from krypy_amd import utils, precond; " \
                   "assert utils.ChebyshevOperator is precond.ChebyshevOperator; print('ok')"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


if __name__ == "__main__":          # records the fixture: meant for the commit named in it only
    rec = record()
    rec["recorded_from_commit"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True,
                                                 text=True).stdout.strip()
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d messages, %d scenarios -> %s" % (len(rec["messages"]), len(rec["scenarios"]), FIXTURE))
