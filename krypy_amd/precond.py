"""Preconditioners built and applied on the device: sparse triangular solves, ILU(0), sparse approximate inverses (SPAI, FSAI),
block-Jacobi and the Chebyshev polynomial.

The reference has no counterpart for anything here - its solvers take any callable as ``M``, ``Ml`` or ``Mr`` - so, unlike
:mod:`krypy_amd.utils`, this module mirrors no file of it.  Every public name is also reachable as ``krypy_amd.utils.NAME``.
"""
import numpy
import scipy.sparse

from . import _hip
from .utils import (ArgumentError, Arnoldi, DeviceOperator, LinearOperator, LinearOperatorError, MatrixLinearOperator, _bdt,
                    _cached, _is_c, _is_sparse, _isintlike)

__all__ = [
    "TriangularSolveOperator", "ilu_operator", "Ilu0Factors", "ilu0", "ilu0_operator", "Ilu0Preconditioner",
    "ilu0_preconditioner", "spai", "spai_operator", "fsai", "fsai_operator", "block_jacobi", "BlockJacobiPreconditioner",
    "block_jacobi_operator", "chebyshev_coefficients", "ChebyshevOperator", "chebyshev_operator",
]


def _two_dim(A, what=""):
    """``A`` itself if it is sparse, else as an ndarray, which has to be 2-D; ``what`` prefixes the message."""
    if not _is_sparse(A):
        A = numpy.asarray(A)
        if A.ndim != 2:
            raise ArgumentError("%sa matrix expected, got an array of shape %s" % (what, A.shape,))
    return A


def _widened(A):
    """``A`` in the device's precision: float32 / complex64 (and integers) become float64 / complex128."""
    if A.dtype in (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)):
        return A
    return A.astype(_bdt(A.dtype))


def _canonical_csr(A, needs=None, what="", square=None, widen=False):
    """The canonical CSR copy of a user's matrix - a sparse matrix, a dense array or, where ``needs`` names the function that
    asks, a :class:`MatrixLinearOperator` that has a host matrix: duplicates summed, indices sorted, stored zeros kept.
    ``what`` prefixes the message for input that is not 2-D; ``square`` is the noun of the message for a matrix that is not
    square (None: any shape passes); ``widen`` makes it float64 / complex128."""
    if needs is not None and isinstance(A, MatrixLinearOperator):
        A = A._A
        if A is None:
            raise ArgumentError("%s needs the matrix: this operator exists on the device only" % needs)
    A = scipy.sparse.csr_matrix(_two_dim(A, what), copy=True)
    if square is not None and A.shape[0] != A.shape[1]:
        raise ArgumentError("a square %s expected, got shape %s" % (square, A.shape,))
    A.sum_duplicates()
    A.sort_indices()
    return _widened(A) if widen else A


def _first_differing_row(A, P):
    """The first row in which the patterns of the canonical CSR matrices ``A`` and ``P`` of one shape differ, or None."""
    if numpy.array_equal(A.indptr, P.indptr) and numpy.array_equal(A.indices, P.indices):
        return None
    n = P.shape[0]
    ptr = numpy.flatnonzero(A.indptr != P.indptr)
    r1 = int(ptr[0]) - 1 if ptr.size else n
    m = int(P.indptr[r1]) if r1 < n else P.nnz          # the rows before r1 start at the same positions
    idx = numpy.flatnonzero(A.indices[:m] != P.indices[:m])
    r2 = int(numpy.searchsorted(P.indptr, idx[0], side="right")) - 1 if idx.size else n
    return min(r1, r2)


class TriangularSolveOperator(LinearOperator):
    """``T^{-1}`` for a sparse triangular matrix ``T``, applied on the device by level-scheduled substitution
    (``Context.tri`` / ``tri_solve``): the factor of an incomplete factorisation or a Gauss-Seidel sweep as ``M``, ``Ml``,
    ``Mr`` or ``ip_B`` of a solver, without a trip over the host.  The reference has no counterpart (it takes any callable).

    ``lower=None`` infers the side from the structure; ``unit_diagonal=True`` takes the diagonal as 1 whatever is stored.
    The result is that of the row-by-row substitution ``s = b_i; s -= t_ij x_j`` (ascending ``j``), ``x_i = s / t_ii``.
    ``_device_matrix()`` stays None: the solvers treat it as an external operator, applied once per step."""

    def __init__(self, T, lower=None, unit_diagonal=False):
        # (widened: the device works in fp64 / c128 and the operator says so)
        T = _canonical_csr(T, square="triangular matrix", widen=True)
        C = T.tocoo()
        below, above = bool(numpy.any(C.row > C.col)), bool(numpy.any(C.row < C.col))
        if lower is None:
            if below and above:
                raise ArgumentError("T is not triangular: entries on both sides of the diagonal")
            lower = not above
        elif (above if lower else below):
            raise ArgumentError("T has entries %s the diagonal, lower=%r" % ("above" if lower else "below", bool(lower)))
        if not unit_diagonal and numpy.any(T.diagonal() == 0):
            raise ArgumentError("T has a zero or missing diagonal entry in row %d (unit_diagonal=False)"
                                % int(numpy.flatnonzero(T.diagonal() == 0)[0]))
        super(TriangularSolveOperator, self).__init__(T.shape, T.dtype, self._dot, self._dot_adj)
        self._T, self.lower, self.unit_diagonal = T, bool(lower), bool(unit_diagonal)
        self._dtris = {}
        self._adj_op = None

    def _device_tri(self, ctx, dtype=None):
        """Device image for blocks of ``dtype``: a real T is created a second time as c128 when it meets complex vectors."""
        return _cached(self._dtris, ctx, _bdt(self.dtype, dtype),
                       lambda dt: ctx.tri(self._T, self.lower, self.unit_diagonal, dtype=dt))

    def _apply_dev(self, X, xcol, Y, ycol, ncols=1):
        self._refuse_real_block(X, "triangular matrix")
        X.ctx.tri_solve(self._device_tri(X.ctx, X.dtype), X, xcol, Y, ycol, ncols)

    _dot = LinearOperator._dot_via_device

    @property
    def adj(self):
        """``(T^H)^{-1}``: the triangular solve with the conjugate transpose, the other triangle."""
        if self._adj_op is None:
            self._adj_op = TriangularSolveOperator(self._T.conj().T, lower=not self.lower, unit_diagonal=self.unit_diagonal)
            self._adj_op._adj_op = self
        return self._adj_op

    def _dot_adj(self, X):
        return self.adj._dot(X)

    def __repr__(self):
        return "<%dx%d TriangularSolveOperator (%s%s) with dtype=%s>" % (
            self.shape[0], self.shape[1], "lower" if self.lower else "upper", ", unit diagonal" if self.unit_diagonal else "",
            self.dtype)


def ilu_operator(ilu):
    """The solve of a sparse LU / incomplete LU factorisation as a device operator: ``ilu`` is any object with ``L``
    (unit lower), ``U`` (upper), ``perm_r`` and ``perm_c`` - what ``scipy.sparse.linalg.spilu`` / ``splu`` return.
    ``ilu.solve(b)`` is ``y[perm_r] = b; z = U^{-1} L^{-1} y; x = z[perm_c]``; the operator is ``Pc * Uinv * Linv * Pr``
    with the two triangular solves on the device and the permutations as CSR matrices of ones (left out when they are the
    identity)."""
    L, U = ilu.L, ilu.U
    n = L.shape[0]
    ar = numpy.arange(n)
    op = TriangularSolveOperator(U, lower=False) * TriangularSolveOperator(L, lower=True, unit_diagonal=True)
    perm_r, perm_c = numpy.asarray(ilu.perm_r), numpy.asarray(ilu.perm_c)
    if not numpy.array_equal(perm_r, ar):
        op = op * MatrixLinearOperator(scipy.sparse.csr_matrix((numpy.ones(n), (perm_r, ar)), shape=(n, n)))
    if not numpy.array_equal(perm_c, ar):
        op = MatrixLinearOperator(scipy.sparse.csr_matrix((numpy.ones(n), (ar, perm_c)), shape=(n, n))) * op
    return op


class Ilu0Factors(object):
    """What :func:`ilu0` returns: the attributes of ``scipy.sparse.linalg.spilu``'s result that :func:`ilu_operator` reads
    (``L`` unit lower with explicit ones, ``U``, ``perm_r``, ``perm_c``, ``shape``, ``nnz``) plus ``info`` and ``solve``."""

    def __init__(self, L, U, perm, info):
        self.L, self.U, self.info = L, U, info
        self.shape = L.shape
        self.nnz = L.nnz + U.nnz
        # solve: x[perm] = U^{-1} L^{-1} b[perm].  ilu_operator computes y[perm_r] = b; z = U^{-1} L^{-1} y; x = z[perm_c]:
        # y = b[perm] and x[perm] = z hold for perm_r = perm_c = the inverse permutation
        inv = numpy.empty_like(perm)
        inv[perm] = numpy.arange(perm.size, dtype=perm.dtype)
        self.perm, self.perm_r, self.perm_c = perm, inv, inv.copy()
        self._op = None

    @property
    def operator(self):
        """The solve as a device operator (:func:`ilu_operator` of this object), built once."""
        if self._op is None:
            self._op = ilu_operator(self)
        return self._op

    def solve(self, b):
        """``x`` with ``x[p] = U^{-1} L^{-1} b[p]`` for one vector or the columns of an ``(n, k)`` array, through the device
        operator."""
        b = numpy.asarray(b)
        x = self.operator.dot(b.reshape(self.shape[0], -1))
        return x.reshape(b.shape) if b.ndim == 1 else x


def _ilu0_check_ordering(ordering):
    if ordering not in ("natural", "multicolor"):
        raise ArgumentError("ordering %r: 'natural' or 'multicolor' expected" % (ordering,))


def _ilu0_canonical(A):
    """The matrix :func:`ilu0` and :class:`Ilu0Preconditioner` factor: a square fp64 / c128 CSR copy with duplicates summed,
    indices sorted, stored zeros kept and a structural diagonal in every row."""
    A = _canonical_csr(A, needs="ilu0", square="matrix", widen=True)
    n = A.shape[0]
    rows = numpy.repeat(numpy.arange(n), numpy.diff(A.indptr))
    has_diag = numpy.zeros(n, dtype=bool)
    has_diag[rows[A.indices == rows]] = True
    if not has_diag.all():
        raise ArgumentError("A has no diagonal entry in row %d: ILU(0) needs a structural diagonal" % int(numpy.flatnonzero(~has_diag)[0]))
    return A


def _ilu0_ordering(A, ordering):
    """``(perm, colors)`` of the canonical ``A``: the identity and None, or the rows sorted by the colours of the greedy
    colouring of ``A + A^T`` and their number."""
    if ordering != "multicolor":
        return numpy.arange(A.shape[0]), None
    G = scipy.sparse.csr_matrix((numpy.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    G = (G + G.T).tocsr()
    G.sort_indices()
    color, ncolors = _hip.multicolor(G)
    return numpy.argsort(color, kind="stable"), ncolors


def _ilu0_breakdown(bad, perm, ordering):
    return ArgumentError("ILU(0) breaks down: zero or non-finite pivot in row %d" % bad
                         + (" (row %d of the original numbering)" % int(perm[bad]) if ordering == "multicolor" else ""))


def ilu0(A, ordering="natural"):
    """ILU(0) of ``A`` - the incomplete LU factorisation on the pattern of ``A`` itself, no pivoting, no fill - computed on the
    device (``Context.ilu0``): an object that quacks like ``scipy.sparse.linalg.spilu``'s result, so :func:`ilu_operator`
    takes it unchanged.  The reference has no counterpart (it takes any callable as a preconditioner).

    ``A``: a SciPy sparse matrix, a dense array or a :class:`MatrixLinearOperator`, square, with a structural diagonal entry
    in every row; stored zeros stay in the pattern.  ``ordering="natural"`` factors ``A`` as it is; ``"multicolor"`` factors
    ``A[p][:, p]`` for the permutation ``p`` that sorts the rows by the colours of a greedy colouring of ``A + A^T`` - rows
    of one colour do not depend on each other, so each factor has as many levels as there are colours (2 for a 5-point
    stencil) where the natural order has as many as the grid has anti-diagonals.  The multicolour factors precondition
    worse: which ordering solves faster is a matter of measurement.  ``solve(b)`` computes ``x[p] = U^{-1} L^{-1} b[p]``.

    Solver hooks: ``Ml`` / ``Mr`` of GMRES for a nonsymmetric ``A``; ``M`` of CG / MINRES for a symmetric ``A``, where
    ILU(0) is ``L D L^T`` and ``M`` is symmetric up to rounding.  Look at ``info["levels"]`` (and, once applied, at the
    ``levels`` of the two triangular operators' ``info()``) before trusting the speed: the factorisation takes one
    launch step per level, and so does every triangular solve.

    ``info``: ``n, nnz, levels, wide_launches, narrow_launches, widest_level, longest_row, first_broken_row`` of the
    factorisation's plan, ``ordering`` and ``colors`` (None for the natural order).  Raises :class:`ArgumentError` for a
    matrix that is not square, a missing diagonal entry, an unknown ordering and a breakdown (a pivot that is zero or
    not finite)."""
    _ilu0_check_ordering(ordering)
    A = _ilu0_canonical(A)
    n = A.shape[0]
    rows = numpy.repeat(numpy.arange(n), numpy.diff(A.indptr))
    perm, ncolors = _ilu0_ordering(A, ordering)
    if ordering == "multicolor":
        inv = numpy.empty_like(perm)
        inv[perm] = numpy.arange(n)
        # A[perm][:, perm] with stored zeros kept: rows gathered, columns renamed, indices sorted again
        cnt = numpy.diff(A.indptr)[perm]
        indptr = numpy.concatenate([[0], numpy.cumsum(cnt)])
        take = numpy.repeat(A.indptr[:-1][perm] - indptr[:-1], cnt) + numpy.arange(A.nnz)
        A = scipy.sparse.csr_matrix((A.data[take], inv[A.indices[take]], indptr), shape=A.shape)
        A.sort_indices()
        rows = numpy.repeat(numpy.arange(n), cnt)
    lu, info = _hip.get_context().ilu0(A)
    if info["first_broken_row"] >= 0:
        raise _ilu0_breakdown(info["first_broken_row"], perm, ordering)
    low, up = A.indices <= rows, A.indices >= rows
    ldata = numpy.where(A.indices == rows, numpy.ones(1, dtype=lu.dtype), lu)[low]
    factors = []
    for mask, data in ((low, ldata), (up, lu[up])):
        ptr = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(rows[mask], minlength=n))])
        factors.append(scipy.sparse.csr_matrix((data, A.indices[mask], ptr), shape=A.shape))
    return Ilu0Factors(factors[0], factors[1], perm, dict(info, ordering=ordering, colors=ncolors))


def ilu0_operator(A, ordering="natural"):
    """``ilu_operator(ilu0(A, ordering))``: the ILU(0) preconditioner of ``A`` as a device operator - factored on the device,
    applied by two level-scheduled triangular solves.  ``Ml`` / ``Mr`` of GMRES for a nonsymmetric ``A``, ``M`` of CG /
    MINRES for a symmetric one (ILU(0) is then ``L D L^T``, symmetric up to rounding); see :func:`ilu0` for the orderings
    and for ``info["levels"]``, the number to look at before trusting the speed."""
    return ilu_operator(ilu0(A, ordering))


class _RebuiltPreconditioner(LinearOperator):
    """What the preconditioners that live on the device through a sequence of matrices of one pattern share: one device handle
    per context and kind of block (a real ``A`` gets a second, c128 handle when it meets complex vectors), built eagerly in the
    constructor so that a breakdown shows there, :meth:`update` for new values, and the state after a failed build.

    A subclass canonicalises ``A`` and hands it to this constructor, and supplies ``_canonical`` (the same canonicalisation,
    for :meth:`update`), ``_create(ctx, dt) -> (handle, info)``, ``_rebuild(handle) -> info`` with the values of ``self._A``,
    ``_breakdown(info)`` (the error of a build that broke down, else None), ``_pattern_error(row)``, ``_solve`` (the name of
    the ``Context`` entry that applies a handle), ``_noun`` and ``_unusable`` (the message after a failed build)."""

    def __init__(self, A):
        super(_RebuiltPreconditioner, self).__init__(A.shape, A.dtype, self._dot)
        self._A = A
        self._handles = {}
        self._broken = None
        self._builds = 0          # builds asked for, failed ones included
        self._device_handle(_hip.get_context(), self.dtype)      # a breakdown shows here

    def _judge(self, info):
        self._builds += 1
        err = self._breakdown(info)
        if err is not None:
            self._broken = err
            raise err

    def _device_handle(self, ctx, dtype=None):
        """Device handle for blocks of ``dtype``, built the first time a context meets that kind of block."""
        def build(dt):
            h, info = self._create(ctx, dt)
            self._judge(info)
            return h
        return _cached(self._handles, ctx, _bdt(self.dtype, dtype), build)

    def _handle(self):
        """The current context's handle of the operator's own dtype, else any."""
        return self._handles.get((id(_hip.get_context()), self.dtype.kind)) or next(iter(self._handles.values()))

    def update(self, A_new):
        """New values on the pattern this object was built with: canonicalised as in the constructor, then every existing
        device handle is rebuilt.  Raises :class:`ArgumentError` for another shape, another kind of values (real / complex),
        another pattern and a breakdown."""
        A = self._canonical(A_new)
        if A.shape != self.shape:
            raise ArgumentError("update: a matrix of shape %s expected, got %s" % (self.shape, A.shape))
        if A.dtype != self.dtype:
            raise ArgumentError("update: %s values for a preconditioner built with %s" % (A.dtype, self.dtype))
        row = _first_differing_row(A, self._A)
        if row is not None:
            raise self._pattern_error(row)
        self._A = A
        self._broken = None
        for h in list(self._handles.values()):
            self._judge(self._rebuild(h))

    def _usable(self):
        if self._broken is not None:
            raise LinearOperatorError(self._unusable % self._broken)

    def _apply_dev(self, X, xcol, Y, ycol, ncols=1):
        self._usable()
        self._refuse_real_block(X, self._noun)
        getattr(X.ctx, self._solve)(self._device_handle(X.ctx, X.dtype), X, xcol, Y, ycol, ncols)

    def _dot(self, X):
        self._usable()
        return self._dot_via_device(X)


class Ilu0Preconditioner(_RebuiltPreconditioner):
    """The ILU(0) preconditioner of ``A`` as ONE device operator that lives through a sequence of systems with the pattern of
    ``A`` (time steps, Newton iterations, :class:`RecyclingGmres`): the analysis runs once (``Context.ilu0_handle``),
    :meth:`update` factors new values with one upload and a few launches (``ilu0_refactor``), the factors never leave the
    device, and an application is one ``ilu0_solve`` - ``x[p] = U^{-1} L^{-1} b[p]`` with the ordering ``p`` inside the two
    triangular stages, no permutation products.  The reference has no counterpart (it takes any callable).

    ``A`` and ``ordering`` as for :func:`ilu0`, which this object agrees with bit for bit (up to the sign of a zero the
    permutation products of :func:`ilu_operator` lose).  ``Ml`` / ``Mr`` of GMRES, ``M`` of CG / MINRES for a symmetric
    ``A``.  No adjoint.  ``_device_matrix()`` stays None: the solvers treat it as an external operator, applied once per
    step.  A breakdown (a pivot that is zero or not finite) raises :class:`ArgumentError` from the constructor and from
    :meth:`update`; after a failed update the object is unusable - applying it raises :class:`LinearOperatorError` - until an
    update succeeds."""

    def __init__(self, A, ordering="natural"):
        _ilu0_check_ordering(ordering)
        A = _ilu0_canonical(A)
        self._ordering = ordering
        self._perm, self._colors = _ilu0_ordering(A, ordering)
        self._pattern = scipy.sparse.csr_matrix((numpy.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
        super(Ilu0Preconditioner, self).__init__(A)              # a breakdown shows here, as in ilu0()

    _canonical = staticmethod(_ilu0_canonical)
    _solve = "ilu0_solve"
    _noun = "ILU(0) preconditioner"
    _unusable = "the last refactorisation broke down (%s): update() with a matrix that factors first"

    @property
    def ordering(self):
        return self._ordering

    @property
    def info(self):
        """The plan of the device handle (``DeviceIlu0.info()``) plus ``ordering``, ``colors`` (None for the natural order)
        and ``refactorisations``, the number of factorisations this object has run."""
        return dict(self._handle().info(), ordering=self._ordering, colors=self._colors, refactorisations=self._builds)

    def _create(self, ctx, dt):
        """(A real ``A`` is factored a second time in complex arithmetic when it meets complex vectors: the quotient rounds
        differently from the real one in the last bit.)"""
        h = ctx.ilu0_handle(self._pattern, None if self._ordering == "natural" else self._perm, dtype=dt)
        return h, self._rebuild(h)

    def _rebuild(self, h):
        return h.ctx.ilu0_refactor(h, self._A.data)

    def _breakdown(self, info):
        bad = info["first_broken_row"]
        return _ilu0_breakdown(bad, self._perm, self._ordering) if bad >= 0 else None

    def _pattern_error(self, row):
        return ArgumentError("update: the pattern differs from the one the preconditioner was built with, first in row %d" % row)

    def __repr__(self):
        return "<%dx%d Ilu0Preconditioner (%s) with dtype=%s>" % (self.shape[0], self.shape[1], self._ordering, self.dtype)


def ilu0_preconditioner(A, ordering="natural"):
    """``Ilu0Preconditioner(A, ordering)``: the persistent ILU(0) preconditioner - see the class; call ``update(A_new)`` on it
    when the values of ``A`` change and its pattern does not."""
    return Ilu0Preconditioner(A, ordering)


_SPAI_MAX_ROW = 32


def _sai_square(A):
    """``A`` as a square canonical CSR matrix of float64 or complex128 (float32 / complex64 widened).  (Block-Jacobi takes it
    too, and with it the "spai" of its message for a device-only operator.)"""
    return _canonical_csr(A, needs="spai", what="A: ", square="matrix", widen=True)


def _sai_pattern(A, pattern):
    """The pattern argument as a canonical CSR matrix of ``A``'s shape: ``A`` itself for None, otherwise the pattern of a sparse
    matrix (stored zeros kept) or the nonzeros of a dense one."""
    if pattern is None:
        return A
    if not (isinstance(pattern, MatrixLinearOperator) or _is_sparse(pattern)):
        pattern = _two_dim(pattern, "pattern: ") != 0
    P = _canonical_csr(pattern, needs="spai", what="pattern: ")
    if P.shape != A.shape:
        raise ArgumentError("a pattern of shape %s expected, got %s" % (A.shape, P.shape))
    return P


def spai(A, pattern=None, side="left", symmetric=False):
    """The sparse approximate inverse of ``A`` on a fixed pattern (static-pattern SPAI), built on the device in one launch
    (``Context.spai``): a ``scipy.sparse.csr_matrix`` ``M`` with ``M.info`` (a dict).  A preconditioner given as a matrix: as
    ``Ml`` / ``Mr`` it is one sparse product per step, as ``M`` the fused Arnoldi step applies it itself.  The reference has no
    counterpart (it takes any callable as a preconditioner).

    ``side="left"`` minimises ``|| I - M A ||_F`` over all ``M`` with the given pattern (for ``Ml``), ``side="right"``
    ``|| I - A M ||_F`` (for ``Mr``; computed as ``spai(A.T, pattern.T, "left").T``, plain transposes on the host).  Every row is
    a small least-squares problem of its own, solved through its normal equations.  ``A``: a SciPy sparse matrix, a dense array
    or a :class:`MatrixLinearOperator`, square; float32 / complex64 are widened.  ``pattern=None`` is the pattern of ``A``
    (stored zeros kept); otherwise any sparse or dense matrix of ``A``'s shape of which only the pattern is read, ``A @ A`` for
    example; at most 32 entries per row (per column for ``side="right"``).

    ``symmetric=True`` returns ``(M + M^H) / 2``, formed on the host - for the ``M`` hook of CG and MINRES with a Hermitian
    ``A``.  Positive definiteness of the result is NOT checked.

    ``info``: ``n, pnnz, qmax, group_width, workgroups, lds_bytes, first_broken_row`` of the device call, ``side`` and
    ``symmetric``.  Raises :class:`ArgumentError` for a matrix that is not square, a pattern of another shape, an unknown
    side, a pattern row with more than 32 entries and a breakdown (the rows of ``A`` a pattern row selects are linearly
    dependent)."""
    if side not in ("left", "right"):
        raise ArgumentError("side %r: 'left' or 'right' expected" % (side,))
    A = _sai_square(A)
    P = _sai_pattern(A, pattern)
    if side == "right":
        A = A.T.tocsr()
        A.sort_indices()
        if pattern is None:
            P = A
        else:
            P = P.T.tocsr()
            P.sort_indices()
    long_rows = numpy.flatnonzero(numpy.diff(P.indptr) > _SPAI_MAX_ROW)
    if long_rows.size:
        i = int(long_rows[0])
        raise ArgumentError("pattern %s %d has %d entries, at most %d are supported"
                            % ("row" if side == "left" else "column", i, int(P.indptr[i + 1] - P.indptr[i]), _SPAI_MAX_ROW))
    data, info = _hip.get_context().spai(A, P)
    bad = info["first_broken_row"]
    if bad >= 0:
        raise ArgumentError("SPAI breaks down: rows of A selected by pattern row %d are linearly dependent" % bad)
    M = scipy.sparse.csr_matrix((data, P.indices.copy(), P.indptr.copy()), shape=A.shape)
    if side == "right":
        M = M.T.tocsr()
        M.sort_indices()
    if symmetric:
        M = ((M + M.conj().T) / 2).tocsr()
        M.sort_indices()
    M.info = dict(info, side=side, symmetric=bool(symmetric))
    return M


def spai_operator(A, **kw):
    """``MatrixLinearOperator(spai(A, **kw))``: the sparse approximate inverse of ``A`` as a device operator - ``Ml`` / ``Mr``
    of GMRES, or, with ``symmetric=True``, ``M`` of CG / MINRES (positive definiteness is not checked); see :func:`spai`."""
    return MatrixLinearOperator(spai(A, **kw))


def _fsai_pattern(A, pattern):
    """``tril(pattern or A)`` with the diagonal added, as a canonical CSR pattern (stored zeros kept)."""
    P = _sai_pattern(A, pattern)
    n = A.shape[0]
    rows = numpy.repeat(numpy.arange(n), numpy.diff(P.indptr))
    low = P.indices <= rows
    ones = numpy.ones(int(low.sum()) + n)
    T = scipy.sparse.csr_matrix((ones, (numpy.concatenate([rows[low], numpy.arange(n)]),
                                        numpy.concatenate([P.indices[low], numpy.arange(n)]))), shape=A.shape)
    T.sum_duplicates()
    T.sort_indices()
    return T


def fsai(A, pattern=None, check=True):
    """The factorized sparse approximate inverse of the Hermitian positive definite ``A`` on a fixed lower-triangular pattern
    (static-pattern FSAI), built on the device in one launch (``Context.fsai``): the lower-triangular
    ``scipy.sparse.csr_matrix`` ``G`` with ``G.info`` (a dict).  ``G`` approximates ``L^-1`` for ``A = L L^H``, so
    ``M = G^H G`` is Hermitian positive definite BY CONSTRUCTION - what the ``M`` hook of CG and MINRES needs - and is applied
    as sparse products; see :func:`fsai_operator`.  ``G A G^H`` has a unit diagonal.  The reference has no counterpart (it
    takes any callable as a preconditioner).

    Every row is a small dense positive definite solve of its own: with the pattern columns ``J`` of row ``i``, the row is
    ``y / sqrt(y_last)``, ``A[J, J] y = e_last``.  The device computes it up to the square root (a root-free Cholesky
    factorisation); the scaling by ``1 / sqrt(d_i)`` is NumPy's, here.  ``A``: a SciPy sparse matrix, a dense array or a
    :class:`MatrixLinearOperator`, square; float32 / complex64 are widened.  The pattern used is the lower triangle of
    ``pattern`` (None: of ``A``; stored zeros kept; only the pattern of a given matrix is read, ``A @ A`` for example) with the
    diagonal added; at most 32 entries per row.

    ``check=True`` verifies that ``A`` is exactly Hermitian.  With ``check=False`` nothing is verified and ONLY THE LOWER
    TRIANGLE of ``A`` is read: the result is that of the Hermitian matrix with this lower triangle.

    ``info``: ``n, pnnz, qmax, group_width, workgroups, lds_bytes, first_broken_row`` of the device call.  Raises
    :class:`ArgumentError` for a matrix that is not square, a pattern of another shape, a pattern row with more than 32 entries
    in its lower triangle, with ``check=True`` a matrix that is not Hermitian, and a breakdown (``A`` is not positive definite:
    a principal submatrix that a pattern row selects has a pivot that is not positive)."""
    A = _sai_square(A)
    P = _fsai_pattern(A, pattern)
    long_rows = numpy.flatnonzero(numpy.diff(P.indptr) > _SPAI_MAX_ROW)
    if long_rows.size:
        i = int(long_rows[0])
        raise ArgumentError("pattern row %d has %d entries in its lower triangle, at most %d are supported"
                            % (i, int(P.indptr[i + 1] - P.indptr[i]), _SPAI_MAX_ROW))
    if check and (A != A.conj().T).nnz:
        raise ArgumentError("A is not Hermitian (check=False reads its lower triangle only)")
    u, d, info = _hip.get_context().fsai(A, P)
    bad = info["first_broken_row"]
    if bad >= 0:
        raise ArgumentError("A is not positive definite: the principal submatrix selected by pattern row %d has a pivot that is "
                            "not positive" % bad)
    scale = 1.0 / numpy.sqrt(d)
    G = scipy.sparse.csr_matrix((u * numpy.repeat(scale, numpy.diff(P.indptr)), P.indices.copy(), P.indptr.copy()), shape=A.shape)
    G.info = dict(info)
    return G


def fsai_operator(A, pattern=None, form="factored", check=True):
    """The preconditioner ``M = G^H G`` of :func:`fsai` as a device operator - Hermitian positive definite by construction:
    ``M`` of CG / MINRES (and of GMRES with ``self_adjoint``).  For GMRES ``Ml = MatrixLinearOperator(G)``,
    ``Mr = MatrixLinearOperator(G^H)`` with ``G = fsai(A)`` split it.

    ``form="factored"``: ``MatrixLinearOperator(G^H) * MatrixLinearOperator(G)`` - two sparse products per application, both on
    the device, no host round trip.  ``form="matrix"``: ``MatrixLinearOperator((G^H @ G).tocsr())`` - one matrix, the form the
    fused step applies itself as ``M``.  The trade is fill: on the five-point Laplacian ``G^H G`` holds 1.15 times (pattern
    ``tril(A)``: 5,719 against 2 x 2,493 entries on a 37 x 23 grid) to 2 times (``tril(A^4)``: 63,763 against 2 x 16,101) the
    entries of the two factors together.  The operator carries ``G`` as ``.G`` and ``G.info`` as ``.info``."""
    if form not in ("factored", "matrix"):
        raise ArgumentError("form %r: 'factored' or 'matrix' expected" % (form,))
    G = fsai(A, pattern=pattern, check=check)
    Gh = G.conj().T.tocsr()
    Gh.sort_indices()
    if form == "factored":
        op = MatrixLinearOperator(Gh) * MatrixLinearOperator(G)
    else:
        M = (Gh @ G).tocsr()
        M.sum_duplicates()
        M.sort_indices()
        op = MatrixLinearOperator(M)
    op.G, op.info = G, G.info
    return op


_BJAC_MAX_BLOCK = 32


def _bjac_blocks(n, block_size, blocks):
    """The partition of ``0 .. n`` as an int32 pointer array, from exactly one of ``block_size`` and ``blocks``."""
    if (block_size is None) == (blocks is None):
        raise ArgumentError("block-Jacobi: exactly one of block_size and blocks expected")
    if block_size is not None:
        if isinstance(block_size, bool) or not isinstance(block_size, (int, numpy.integer)):
            raise ArgumentError("block_size %r: an integer in 1 .. %d expected" % (block_size, _BJAC_MAX_BLOCK))
        if not 1 <= block_size <= _BJAC_MAX_BLOCK:
            raise ArgumentError("block_size %d: an integer in 1 .. %d expected" % (block_size, _BJAC_MAX_BLOCK))
        ptr = numpy.arange(0, n, int(block_size), dtype=numpy.int64)
        return numpy.concatenate([ptr, [n]]).astype(numpy.int32)
    ptr = numpy.asarray(blocks)
    if ptr.ndim != 1 or ptr.size < 2 or ptr.dtype.kind not in "iu":
        raise ArgumentError("blocks: an integer pointer array with at least two entries expected")
    ptr = ptr.astype(numpy.int64)
    if ptr[0] != 0:
        raise ArgumentError("blocks: the pointer array starts at %d, not at 0" % ptr[0])
    if ptr[-1] != n:
        raise ArgumentError("blocks: the pointer array ends at %d, not at n = %d" % (ptr[-1], n))
    m = numpy.diff(ptr)
    bad = numpy.flatnonzero(m < 1)
    if bad.size:
        raise ArgumentError("blocks: the pointer array is not strictly increasing at block %d" % bad[0])
    bad = numpy.flatnonzero(m > _BJAC_MAX_BLOCK)
    if bad.size:
        raise ArgumentError("blocks: block %d has %d rows, at most %d are supported" % (bad[0], m[bad[0]], _BJAC_MAX_BLOCK))
    return ptr.astype(numpy.int32)


def _bjac_breakdown(bad, blkptr):
    return ArgumentError("block-Jacobi breaks down: diagonal block %d (rows %d .. %d) is singular or not finite"
                         % (bad, blkptr[bad], blkptr[bad + 1] - 1))


def _bjac_csr(values, blkptr, n):
    """The block-diagonal CSR matrix with all ``m_g^2`` entries of every block, from the flat row-major blocks."""
    ptr = blkptr.astype(numpy.int64)
    m = numpy.diff(ptr)
    row_len = numpy.repeat(m, m)                                  # per row: the size of its block
    indptr = numpy.concatenate([[0], numpy.cumsum(row_len)])
    first = numpy.repeat(numpy.repeat(ptr[:-1], m), row_len)      # per entry: the first column of its block
    indices = numpy.arange(indptr[-1]) - numpy.repeat(indptr[:-1], row_len) + first
    return scipy.sparse.csr_matrix((values, indices.astype(numpy.int32), indptr.astype(numpy.int32)), shape=(n, n))


def block_jacobi(A, block_size=None, blocks=None):
    """The block-Jacobi preconditioner of ``A`` as a matrix: the block-diagonal ``scipy.sparse.csr_matrix`` ``M`` whose
    diagonal blocks are the inverses of those of ``A``, inverted on the device in one launch (``Context.bjac_create``,
    Gauss-Jordan elimination with row pivoting), with ``M.info`` (a dict).  All ``m_g^2`` entries of every block are stored
    (zeros too) and the indices are sorted.  The reference has no counterpart (it takes any callable as a preconditioner).

    ``A``: a SciPy sparse matrix, a dense array or a :class:`MatrixLinearOperator`, square; float32 / complex64 are widened;
    entries of a diagonal block that ``A`` does not store are 0.  Exactly one of ``block_size`` - an integer in 1 .. 32, the
    blocks are consecutive ranges of that many rows and the last one may be shorter - and ``blocks`` - the pointer array of the
    partition, ``blocks[0] = 0 < ... < blocks[-1] = n`` with blocks of at most 32 rows - is given.  ``block_size=1`` is point
    Jacobi, ``1.0 / A.diagonal()`` exactly.

    For a Hermitian positive definite ``A`` the result is the ``M`` of CG / MINRES; neither positive definiteness nor the exact
    symmetry of the computed inverse (it is Hermitian up to rounding only) is checked.

    ``info``: ``n, nnz, nblk, max_block, group_width, workgroups, device_bytes, first_broken_block`` of the device call.  Raises
    :class:`ArgumentError` for a matrix that is not square, a bad ``block_size`` / ``blocks`` and a broken block (a pivot that is
    zero or not finite; the smallest such block is named)."""
    A = _sai_square(A)
    blkptr = _bjac_blocks(A.shape[0], block_size, blocks)
    ctx = _hip.get_context()
    h, info = ctx.bjac_create(A, blkptr)
    bad = info["first_broken_block"]
    if bad >= 0:
        raise _bjac_breakdown(bad, blkptr)
    M = _bjac_csr(ctx.bjac_values(h), blkptr, A.shape[0])
    M.info = dict(info)
    return M


class BlockJacobiPreconditioner(_RebuiltPreconditioner):
    """The block-Jacobi preconditioner of ``A`` as ONE device operator: the inverses of the diagonal blocks stay on the device
    in the layout of their own apply kernel (``Context.bjac_create`` / ``bjac_apply``: one streaming launch per column, 8 m
    bytes per row where the same blocks as a CSR matrix cost 12 m + 4), and :meth:`update` rebuilds them for new values on the
    same pattern with one upload and one launch.  The reference has no counterpart (it takes any callable).

    ``A``, ``block_size`` and ``blocks`` as for :func:`block_jacobi`, whose matrix this object agrees with bit for bit - in the
    blocks and in every application.  ``Ml`` / ``Mr`` of GMRES, BiCGStab and IDR(s); ``M`` of CG / MINRES for a Hermitian
    positive definite ``A`` - neither positive definiteness nor the exact symmetry of the computed inverse is checked.  No
    adjoint.  ``_device_matrix()`` stays None: the solvers treat it as an external operator, applied once per step (the fused
    Arnoldi step takes the matrix form, ``block_jacobi_operator(A, ..., form="matrix")``).  A broken block (a pivot that is zero
    or not finite) raises :class:`ArgumentError` from the constructor and from :meth:`update`; after a failed update the object
    is unusable - applying it raises :class:`LinearOperatorError` - until an update succeeds."""

    def __init__(self, A, block_size=None, blocks=None):
        A = _sai_square(A)
        self._blkptr = _bjac_blocks(A.shape[0], block_size, blocks)
        super(BlockJacobiPreconditioner, self).__init__(A)       # a broken block shows here, as in block_jacobi()

    _canonical = staticmethod(_sai_square)
    _solve = "bjac_apply"
    _noun = "block-Jacobi preconditioner"
    _unusable = "the last build broke down (%s): update() with a matrix whose blocks invert first"

    @property
    def blocks(self):
        """The pointer array of the partition."""
        return self._blkptr.copy()

    @property
    def info(self):
        """The figures of the device handle's last build (``DeviceBjac.info()``) plus ``builds``, the number of build
        launches this object has asked for."""
        return dict(self._handle().info(), builds=self._builds)

    def _create(self, ctx, dt):
        return ctx.bjac_create(self._A if dt == self.dtype else self._A.astype(dt), self._blkptr)

    def _rebuild(self, h):
        return h.ctx.bjac_update(h, self._A.data.astype(h.dtype))

    def _breakdown(self, info):
        bad = info["first_broken_block"]
        return _bjac_breakdown(bad, self._blkptr) if bad >= 0 else None

    def _pattern_error(self, row):
        return ArgumentError("update: the pattern differs from the one the preconditioner was built with")

    def matrix(self):
        """The inverse blocks as the block-diagonal CSR matrix of :func:`block_jacobi` (downloaded from the device)."""
        self._usable()
        h = self._handle()
        return _bjac_csr(h.ctx.bjac_values(h), self._blkptr, self.shape[0])

    def __repr__(self):
        return "<%dx%d BlockJacobiPreconditioner (%d blocks) with dtype=%s>" % (self.shape[0], self.shape[1],
                                                                                self._blkptr.size - 1, self.dtype)


def block_jacobi_operator(A, block_size=None, blocks=None, form="blocks"):
    """The block-Jacobi preconditioner of ``A`` as a device operator; ``A``, ``block_size`` and ``blocks`` as for
    :func:`block_jacobi`.  ``form="blocks"`` (default) is :class:`BlockJacobiPreconditioner`, applied by its own kernel;
    ``form="matrix"`` is ``MatrixLinearOperator(block_jacobi(...))``, applied by the CSR kernels - the form the fused Arnoldi
    step takes as ``M``.  Both give the same bits in every application.  ``Ml`` / ``Mr`` of GMRES, BiCGStab and IDR(s), ``M`` of
    CG / MINRES for a Hermitian positive definite ``A`` (positive definiteness and the exact symmetry of the computed inverse
    are not checked)."""
    if form not in ("blocks", "matrix"):
        raise ArgumentError("form %r: 'blocks' or 'matrix' expected" % (form,))
    if form == "matrix":
        return MatrixLinearOperator(block_jacobi(A, block_size, blocks))
    return BlockJacobiPreconditioner(A, block_size, blocks)


def chebyshev_coefficients(lmin, lmax, degree):
    """The ``(degree, 2)`` float64 array of ``(a_k, b_k)`` of the Chebyshev iteration on ``[lmin, lmax]``, in Python floats:
    ``theta = (lmax + lmin) / 2; delta = (lmax - lmin) / 2; sigma = theta / delta; rho_0 = 1 / sigma; (a_0, b_0) = (0, 1 / theta);
    rho_k = 1 / (2 sigma - rho_{k-1}); (a_k, b_k) = (rho_k rho_{k-1}, 2 rho_k / delta)``."""
    lmin, lmax = float(lmin), float(lmax)
    theta = (lmax + lmin) / 2
    delta = (lmax - lmin) / 2
    sigma = theta / delta
    rho = 1 / sigma
    coef = numpy.zeros((degree, 2))
    coef[0] = (0.0, 1 / theta)
    for k in range(1, degree):
        rho_new = 1 / (2 * sigma - rho)
        coef[k] = (rho_new * rho, 2 * rho_new / delta)
        rho = rho_new
    return coef


class ChebyshevOperator(LinearOperator):
    """The Chebyshev polynomial preconditioner ``M = p(A)``: ``z = M r`` is ``degree`` steps of the Chebyshev iteration for
    ``A z = r`` from ``z = 0`` (``Context.cheb_apply`` / ``cheb_update``), for a Hermitian positive definite ``A`` whose
    spectrum lies in ``[lmin, lmax]``.  ``M`` is Hermitian positive definite too, so it serves ``Cg`` and ``Minres`` as ``M``
    and ``Gmres`` as ``M``, ``Ml`` or ``Mr``; it costs ``degree - 1`` applications of ``A`` and consists of operator
    applications and row-local updates only - no factorisation, and it works on a sharded operator.  The reference has no
    counterpart (it takes any callable).

    :param A: a matrix, a ``MatrixLinearOperator`` / ``DeviceOperator`` (all steps in one call of the library, one launch per
        step where the fused kernels apply), or any other ``LinearOperator`` with a device action (one ``A._apply_dev`` and one
        ``cheb_update`` per step).
    :param lmax, lmin: bounds of the spectrum, ``0 < lmin < lmax``; ``lmin`` defaults to ``lmax / ratio``.
    :param degree: number of steps ``m >= 1``.
    :param scale: None, ``"jacobi"`` (the diagonal of a matrix ``A``) or a 1-D array of positive reals ``s``: the iteration
        then runs for ``diag(1/s) A`` and the bounds refer to that operator.

    Per row, every operation rounded on its own: step 0 ``t = r; [t = t * dinv;] d = b_0 * t; z = d``, step k
    ``t = r - A z; [t = t * dinv;] d = (a_k * d) + (b_k * t); z = z + d`` with ``coefficients[k] = (a_k, b_k)``.
    ``_device_matrix()`` stays None: the solvers treat it as an external operator, applied once per step."""

    def __init__(self, A, lmax, lmin=None, degree=4, ratio=30.0, scale=None):
        mat = None
        if isinstance(A, LinearOperator):
            op = A
            if isinstance(A, MatrixLinearOperator) and not isinstance(A, DeviceOperator):
                mat = A._A
        else:
            # (no canonical CSR copy: a dense matrix stays dense and is applied by the dense kernels)
            mat = _two_dim(A)
            if mat.shape[0] == mat.shape[1]:
                mat = _widened(mat)                    # the device works in fp64 / c128 and the operator says so
            op = MatrixLinearOperator(mat)
        if op.shape[0] != op.shape[1]:
            raise ArgumentError("a square operator expected, got shape %s" % (op.shape,))
        if not _isintlike(degree) or degree < 1:
            raise ArgumentError("degree %r: an integer >= 1 expected" % (degree,))
        if lmin is None:
            lmin = float(lmax) / float(ratio)
        lmax, lmin = float(lmax), float(lmin)
        if not (0.0 < lmin < lmax and numpy.isfinite(lmax)):
            raise ArgumentError("bounds 0 < lmin < lmax expected, got lmin = %r, lmax = %r" % (lmin, lmax))
        n = op.shape[0]
        dinv = None
        if scale is not None:
            if isinstance(scale, str):
                if scale != "jacobi":
                    raise ArgumentError("scale %r: None, 'jacobi' or a 1-D array expected" % (scale,))
                if mat is None:
                    raise ArgumentError("scale='jacobi' needs a matrix: this operator has no diagonal to read")
                s = mat.diagonal() if _is_sparse(mat) else numpy.diagonal(numpy.asarray(mat))
            else:
                s = scale
            s = numpy.asarray(s)
            if s.ndim != 1 or s.shape[0] != n:
                raise ArgumentError("a scale of shape (%d,) expected, got %s" % (n, s.shape))
            if s.dtype.kind == "c":
                if numpy.any(s.imag != 0):
                    raise ArgumentError("the scale has a complex entry")
                s = s.real
            s = numpy.asarray(s, dtype=float)
            if not numpy.all(s > 0) or not numpy.all(numpy.isfinite(s)):
                raise ArgumentError("the scale has an entry that is not a positive finite number")
            dinv = 1.0 / s
        super(ChebyshevOperator, self).__init__((n, n), _bdt(op.dtype), self._dot, self._dot)
        self._op, self._matrix_path = op, isinstance(op, MatrixLinearOperator)
        self.degree, self.lmin, self.lmax = int(degree), lmin, lmax
        self.coefficients = chebyshev_coefficients(lmin, lmax, self.degree)
        self.dinv = dinv
        self._dinv_dev = {}
        self._blocks = {}

    @property
    def adj(self):
        """The operator itself: ``p(A)`` with real coefficients is Hermitian when ``A`` is."""
        return self

    def _dinv_image(self, ctx, dtype):
        """``dinv`` as a real device diagonal: of length N for real blocks, 2N (every entry twice) for the (re, im) view."""
        if self.dinv is None:
            return None
        return _cached(self._dinv_dev, ctx, _bdt(dtype),
                       lambda dt: ctx.diag(numpy.repeat(self.dinv, 2) if _is_c(dt) else self.dinv))

    def _cheb_scratch(self, ctx, dtype):
        """Three columns per context and block dtype: d, the other half of the z ping-pong, A z."""
        return _cached(self._blocks, ctx, _bdt(dtype), lambda dt: ctx.alloc(self.shape[0], 3, dtype=dt))

    def _apply_dev(self, X, xcol, Y, ycol, ncols=1):
        self._refuse_real_block(X, "Chebyshev operator")
        ctx = X.ctx
        S = self._cheb_scratch(ctx, X.dtype)
        dinv = self._dinv_image(ctx, X.dtype)
        if X is Y and xcol < ycol + ncols and ycol < xcol + ncols:      # r is read in every step: it moves out of the result's way
            T = ctx.alloc(X.n, ncols, dtype=X.dtype)
            T.copy_from(0, X, xcol, ncols)
            X, xcol = T, 0
        if self._matrix_path:
            dm = self._op._device_matrix(ctx, X.dtype)
            if dm.kind != "diag":                  # (a diagonal A goes the general way: kh_cheb_apply takes CSR and dense handles)
                ctx.cheb_apply(dm, dinv, self.coefficients, X, xcol, Y, ycol, ncols, S)
                return
        coef, m = self.coefficients, self.degree
        for c in range(ncols):
            # z after step k lives in Y when m - 1 - k is even, else in the scratch: the last step lands in Y
            where = [(Y, ycol + c) if (m - 1 - k) % 2 == 0 else (S, 1) for k in range(m)]
            ctx.cheb_update(None, 0, X, xcol + c, dinv, S, 0, None, 0, where[0][0], where[0][1], 0.0, coef[0, 1], first=True)
            for k in range(1, m):
                (Zi, zi), (Zo, zo) = where[k - 1], where[k]
                self._op._apply_dev(Zi, zi, S, 2, 1)
                ctx.cheb_update(S, 2, X, xcol + c, dinv, S, 0, Zi, zi, Zo, zo, coef[k, 0], coef[k, 1])

    _dot = LinearOperator._dot_via_device

    def __repr__(self):
        return "<%dx%d ChebyshevOperator (degree %d on [%g, %g]%s) with dtype=%s>" % (
            self.shape[0], self.shape[1], self.degree, self.lmin, self.lmax, "" if self.dinv is None else ", scaled", self.dtype)


def chebyshev_operator(A, degree=4, steps=10, boost=1.1, ratio=30.0, scale=None, seed=0):
    """A :class:`ChebyshevOperator` with an estimated upper bound: ``lmax = boost *`` the largest Ritz value of ``steps``
    Lanczos steps (``Arnoldi(..., ortho='lanczos')`` on the device, the eigenvalues of the tridiagonal matrix on the host) on
    ``A``, or on ``D^{-1/2} A D^{-1/2}`` when scaled (the spectrum of ``D^{-1} A``), from a seeded normal start vector;
    ``lmin = lmax / ratio``.  The estimate is kept as ``lmax_estimate``."""
    probe = ChebyshevOperator(A, 1.0, degree=degree, ratio=ratio, scale=scale)       # the argument checks, op and dinv
    op = probe._op
    n = op.shape[0]
    if probe.dinv is not None:
        Dh = MatrixLinearOperator(scipy.sparse.diags(numpy.sqrt(probe.dinv)).tocsr())
        op = Dh * op * Dh
    v = numpy.random.default_rng(seed).standard_normal((n, 1))
    if _is_c(op.dtype):
        v = v.astype(complex)
    arn = Arnoldi(op, v, maxiter=min(int(steps), n), ortho="lanczos")
    while arn.iter < arn.maxiter and not arn.invariant:
        arn.advance()
    k = arn.iter
    H = numpy.asarray(arn.H[:k, :k])
    theta = numpy.linalg.eigvalsh((H + H.conj().T) / 2)
    lmax = float(boost) * float(theta[-1])
    out = ChebyshevOperator(A, lmax, degree=degree, ratio=ratio, scale=scale)
    out.lmax_estimate = lmax
    return out

