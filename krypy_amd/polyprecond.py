"""The GMRES polynomial preconditioner ``p(A) ~ A^-1`` of Loe & Morgan for non-symmetric and indefinite operators: the roots of
``1 - z p(z)`` are the harmonic Ritz values of ``degree`` Arnoldi steps, so it needs no spectral bounds, and it consists of
operator applications and row-local updates only - no factorisation, and it works on shards and communicators.

The reference has no counterpart - its solvers take any callable as ``M``, ``Ml`` or ``Mr`` - so this module mirrors no file of
it.  The public names are also reachable as ``krypy_amd.utils.NAME``.

    J. A. Loe, R. B. Morgan: Toward efficient polynomial preconditioning for GMRES.  Numer. Linear Algebra Appl. 29 (2022).
"""
import math
import warnings

import numpy

from .precond import _two_dim, _widened
from .utils import (ArgumentError, Arnoldi, DeviceOperator, LinearOperator, LinearOperatorError, MatrixLinearOperator, _cached,
                    _is_c, _isintlike)

__all__ = ["gmres_polynomial_roots", "gmres_polynomial_steps", "GmresPolynomialOperator", "gmres_polynomial_operator"]

LIN, QA, QB, SCALE = 0, 1, 2, 3
_POF_WARN = 4.0      # log10 of the product of factors above which the polynomial is unreliable in double precision


def _operator_of(A):
    """``A`` as a real square ``LinearOperator``: a matrix becomes a ``MatrixLinearOperator`` (widened to fp64, a dense matrix
    stays dense)."""
    if isinstance(A, LinearOperator):
        op = A
    else:
        mat = _two_dim(A)
        if mat.shape[0] == mat.shape[1]:
            mat = _widened(mat)
        op = MatrixLinearOperator(mat)
    if op.shape[0] != op.shape[1]:
        raise ArgumentError("a square operator expected, got shape %s" % (op.shape,))
    if _is_c(op.dtype):
        raise NotImplementedError("the GMRES polynomial preconditioner takes real operators on real blocks only, got dtype %s"
                                  % (op.dtype,))
    return op


def _log(x):
    return math.log(x) if x > 0.0 else -math.inf


def _leja(theta):
    """The modified Leja order of roots that ``eigvals`` returned (real ones with imaginary part exactly 0, pairs exactly
    conjugate): candidates are the real roots and the ``Im > 0`` member of each pair; first the one of largest modulus, then
    the one that maximises ``sum log |theta - mu|`` over all roots ``mu`` placed so far; ties go to the candidate returned
    first; a pair's conjugate follows its ``Im > 0`` member immediately."""
    cand = [complex(t) for t in theta if complex(t).imag >= 0.0]
    placed = []
    score = [abs(t) for t in cand]
    while cand:
        best = 0
        for j in range(1, len(cand)):
            if score[j] > score[best]:
                best = j
        t = cand.pop(best)
        placed.append(t)
        if t.imag != 0.0:
            placed.append(t.conjugate())
        score = []
        for u in cand:
            s = 0.0
            for mu in placed:
                s = s + _log(abs(u - mu))
            score.append(s)
    return numpy.array(placed, dtype=complex)


def _log10_pof_max(theta):
    """``max_k log10 prod_{i != k} |1 - theta_k / theta_i|``, the product accumulated as a sum of logs."""
    theta = [complex(t) for t in theta]            # (Python's complex division, not NumPy's)
    worst = -math.inf
    for k, tk in enumerate(theta):
        s = 0.0
        for i, ti in enumerate(theta):
            if i != k:
                s = s + _log(abs(1.0 - tk / ti))
        worst = max(worst, s / math.log(10.0))
    return worst


def gmres_polynomial_roots(A, degree=8, v=None, seed=0):
    """``(roots, info)``: the roots of the GMRES residual polynomial of ``degree`` Arnoldi steps (``Arnoldi(A, v,
    ortho='mgs')`` on the device) in modified Leja order - the harmonic Ritz values, on the host
    ``eigvals(H_d + h_{d+1,d}^2 f e_d^T)`` with ``f = H_d^{-H} e_d``.  ``v`` defaults to the seeded normal vector
    ``numpy.random.default_rng(seed).standard_normal((n, 1))``.  An invariant subspace at step ``k < degree`` gives
    ``eigvals(H_k)``.  A root is real iff its imaginary part is exactly 0.

    ``info``: ``degree`` (the number of roots), ``log10_pof_max`` - the largest ``log10`` of the products
    ``pof(k) = prod_{i != k} |1 - theta_k / theta_i|``; above 4 the polynomial is unreliable in double precision and a warning
    is issued (adding roots for stability is not implemented)."""
    op = _operator_of(A)
    n = op.shape[0]
    if not _isintlike(degree) or degree < 1:
        raise ArgumentError("degree %r: an integer >= 1 expected" % (degree,))
    if v is None:
        v = numpy.random.default_rng(seed).standard_normal((n, 1))
    v = numpy.asarray(v, dtype=float).reshape(n, 1)
    d = min(int(degree), n)
    arn = Arnoldi(op, v, maxiter=d, ortho="mgs")
    while arn.iter < arn.maxiter and not arn.invariant:
        arn.advance()
    k = arn.iter
    H = numpy.array(arn.H[:k + 1, :k], dtype=float)
    if arn.invariant or k < int(degree):
        theta = numpy.linalg.eigvals(H[:k, :k])
    else:
        Hd = H[:k, :k]
        e = numpy.zeros(k)
        e[-1] = 1.0
        try:
            f = numpy.linalg.solve(Hd.T, e)
        except numpy.linalg.LinAlgError:
            f = None
        if f is None or not numpy.all(numpy.isfinite(f)):
            raise ArgumentError("the Hessenberg matrix of %d Arnoldi steps is singular: no harmonic Ritz values" % k)
        G = Hd.copy()
        G[:, -1] = G[:, -1] + (H[k, k - 1] * H[k, k - 1]) * f
        theta = numpy.linalg.eigvals(G)
    roots = _leja(theta)
    gmres_polynomial_steps(roots)                  # (refuses zero and non-finite roots)
    info = dict(degree=int(roots.shape[0]), log10_pof_max=_log10_pof_max(roots))
    if info["log10_pof_max"] > _POF_WARN:
        warnings.warn("GMRES polynomial of degree %d: log10 pof = %.1f > %g, the polynomial is unreliable at this degree"
                      % (info["degree"], info["log10_pof_max"], _POF_WARN))
    return roots, info


def gmres_polynomial_steps(roots):
    """The ``(nsteps, 5)`` float64 table of ``(kind, c, a2, close, cl)`` for ordered ``roots`` (a pair's members adjacent), all
    entries in Python floats.  A real root that is not the last: LIN (kind 0) with ``c = 1 / theta``; the last root, real: no
    step of its own, the previous step gets ``close = 1, cl = 1 / theta``; the only root: one SCALE (kind 3) row; a pair
    ``a +- ib``: QA (kind 1) with ``a2 = 2 a, c = 1 / ((a * a) + (b * b))``, then QB (kind 2) with the same ``c`` unless the pair
    is last.  ``degree - 1`` rows for ``degree >= 2``, one operator application each."""
    theta = [complex(t) for t in numpy.asarray(roots).reshape(-1)]
    d = len(theta)
    if d < 1:
        raise ArgumentError("at least one root expected")
    for t in theta:
        if not (math.isfinite(t.real) and math.isfinite(t.imag)):
            raise ArgumentError("a root is not finite: %r" % (t,))
        if t == 0:
            raise ArgumentError("a root is zero: p(A) does not exist")
    rows = []
    i = 0
    while i < d:
        t = theta[i]
        if t.imag == 0.0:
            r = t.real
            if i < d - 1:
                rows.append([LIN, 1 / r, 0.0, 0.0, 0.0])
            elif d == 1:
                rows.append([SCALE, 1 / r, 0.0, 0.0, 0.0])
            else:
                rows[-1][3], rows[-1][4] = 1.0, 1 / r
            i += 1
        else:
            if i + 1 >= d or theta[i + 1] != t.conjugate():
                raise ArgumentError("the roots are not closed under conjugation: %r is not followed by its conjugate" % (t,))
            a, b = t.real, t.imag
            c = 1 / ((a * a) + (b * b))
            rows.append([QA, c, 2 * a, 0.0, 0.0])
            if i + 2 < d:
                rows.append([QB, c, 0.0, 0.0, 0.0])
            i += 2
    return numpy.array(rows, dtype=numpy.float64).reshape(len(rows), 5)


class GmresPolynomialOperator(LinearOperator):
    """The GMRES polynomial preconditioner ``M = p(A)`` with ``1 - z p(z) = prod (1 - z / theta_i)`` for given ``roots``
    (:func:`gmres_polynomial_roots`; closed under conjugation, a pair's members adjacent), applied in the product form: real
    roots as linear factors, conjugate pairs as real quadratic ones, ``degree - 1`` applications of ``A``
    (``Context.poly_apply`` / ``poly_update``).  For non-symmetric and indefinite ``A``; it serves ``Gmres``,
    ``RestartedGmres``, ``Bicgstab`` and ``Idrs`` as ``Ml`` or ``Mr``.  As ``M`` of ``Cg`` / ``Minres`` it is the caller's
    responsibility that ``p`` is positive on the spectrum.  Real operators on real blocks only.  The reference has no
    counterpart (it takes any callable).

    :param A: a matrix, a ``MatrixLinearOperator`` / ``DeviceOperator`` (all steps in one call of the library, one launch per
        step where the fused kernels apply), or any other ``LinearOperator`` with a device action (one ``A._apply_dev`` and one
        ``poly_update`` per step).
    :param roots: the ordered roots.

    Attributes: ``roots``, ``steps`` (the table of :func:`gmres_polynomial_steps`), ``degree``, ``info``.  Per row, with
    ``s = (A in)_i`` and every operation rounded on its own: LIN ``y = y + (c * in); out = in - (c * s)``, QA
    ``t = (a2 * in) - s; y = y + (c * t); out = t``, QB ``out = prod - (c * s)``; the first step does not read ``y``; a closing
    real root adds ``y = y + (cl * out)``.  ``_device_matrix()`` stays None: the solvers treat it as an external operator."""

    def __init__(self, A, roots, info=None):
        op = _operator_of(A)
        n = op.shape[0]
        self.roots = numpy.array(roots, dtype=complex).reshape(-1)
        self.steps = gmres_polynomial_steps(self.roots)
        super(GmresPolynomialOperator, self).__init__((n, n), numpy.dtype(float), self._dot, None)
        self._op = op
        self._matrix_path = isinstance(op, (MatrixLinearOperator, DeviceOperator))
        self.degree = int(self.roots.shape[0])
        self.info = dict(degree=self.degree) if info is None else dict(info)
        self._blocks = {}

    def _poly_scratch(self, ctx, dtype):
        """Three columns per context and block dtype: the two halves of the prod ping-pong, t."""
        return _cached(self._blocks, ctx, numpy.dtype(dtype), lambda dt: ctx.alloc(self.shape[0], 3, dtype=dt))

    def _apply_dev(self, X, xcol, Y, ycol, ncols=1):
        if _is_c(X.dtype):
            raise LinearOperatorError("real GMRES polynomial operator applied to a complex device block")
        ctx = X.ctx
        S = self._poly_scratch(ctx, X.dtype)
        if X is Y and xcol < ycol + ncols and ycol < xcol + ncols:      # x is read by every step: it moves out of the result's way
            T = ctx.alloc(X.n, ncols, dtype=X.dtype)
            T.copy_from(0, X, xcol, ncols)
            X, xcol = T, 0
        if self._matrix_path:
            dm = self._op._device_matrix(ctx, X.dtype)
            if dm.kind != "diag":                  # (a diagonal A goes the general way: kh_poly_apply takes CSR and dense handles)
                ctx.poly_apply(dm, self.steps, X, xcol, Y, ycol, ncols, S)
                return
        for c in range(ncols):
            if int(self.steps[0, 0]) == SCALE:
                ctx.poly_update(X, xcol + c, None, 0, Y, ycol + c, None, 0, SCALE, self.steps[0, 1], first=True)
                continue
            p = -1                                  # where prod is: -1 x itself, then scratch column 0 / 1; t lives in column 2
            where = lambda col: (X, xcol + c) if col < 0 else (S, col)      # noqa: E731
            for k, (kind, cc, a2, close, cl) in enumerate(self.steps):
                kind = int(kind)
                other = 1 if p == 0 else 0
                (I, icol), out = where(2 if kind == QB else p), (2 if kind == QA else other)
                P, pcol = where(p) if kind == QB else (None, 0)
                self._op._apply_dev(I, icol, S, out, 1)
                ctx.poly_update(I, icol, P, pcol, Y, ycol + c, S, out, kind, cc, a2, cl, first=k == 0, close=close != 0.0)
                if kind != QA:
                    p = other

    _dot = LinearOperator._dot_via_device

    def __repr__(self):
        return "<%dx%d GmresPolynomialOperator (degree %d, %d real roots, %d pairs) with dtype=%s>" % (
            self.shape[0], self.shape[1], self.degree, int(numpy.sum(self.roots.imag == 0)),
            int(numpy.sum(self.roots.imag > 0)), self.dtype)


def gmres_polynomial_operator(A, degree=8, v=None, seed=0):
    """A :class:`GmresPolynomialOperator` whose roots are the harmonic Ritz values of ``degree`` Arnoldi steps on ``A`` from ``v``
    (default: a seeded normal vector), :func:`gmres_polynomial_roots`; its ``info`` is that function's."""
    op = _operator_of(A)
    roots, info = gmres_polynomial_roots(op, degree=degree, v=v, seed=seed)
    return GmresPolynomialOperator(op, roots, info)
