"""Helpers of the poisoned-block tests (tests/test_gpu_poison.py, one CPU test in tests/test_host_logic.py) -
TEST INFRASTRUCTURE ONLY, importable without a GPU.

Two storage contracts carry the fast kernels: (1) a block asked for with ``zero=False`` may hold anything, so every
column is written before it is read; (2) the padding of a block (rows ``[n, ld)`` of every column, the slack behind the
last column) is zero and no kernel ever writes there.  ``poison`` / ``poisoned_allocations`` make a violation of (1)
visible (a NaN that is read reaches a result), ``DeviceVectors.padding_nonzero`` reads what (2) promises, ``bits_equal``
compares results so that NaN != NaN hides nothing, and ``arnoldi_longdouble`` is a reference of the Arnoldi step that
shares no code with the library or with ``oracle/``."""
import contextlib
import weakref

import numpy as np
import scipy.sparse as sp


def poison(block, cols=None, value=np.nan):
    """Overwrite rows ``[0, n)`` of the columns ``cols`` (default: all) of a device block with ``value`` (a quiet NaN).
    Goes through ``upload``, which writes exactly ``n`` rows per column: the padding is not touched.  One n-vector on
    the host, uploaded column by column."""
    cols = range(block.ncols) if cols is None else cols
    fill = np.full(block.n, value, dtype=block.dtype)
    if block.dtype.kind == "c":
        fill.imag = value
    for c in cols:
        block.upload(c, fill)
    return block


class _Record(object):
    """What ``poisoned_allocations`` handed out: weak references, so that a dropped block still goes back to the pool."""

    def __init__(self):
        self._refs = []
        self.poisoned = 0

    def add(self, block):
        self._refs.append(weakref.ref(block))

    def live(self):
        return [b for b in (r() for r in self._refs) if b is not None and getattr(b, "handle", None) is not None]


@contextlib.contextmanager
def poisoned_allocations(ctx, value=np.nan):
    """Inside the ``with``, every block ``ctx.alloc`` is asked for with ``zero=False`` - fresh or from the pool - is
    poisoned before it is returned; every block handed out (zero-filled ones too) is recorded.  Yields the record
    (``live()``: the blocks that still exist, ``poisoned``: how many were filled).  The original ``alloc`` is back on
    exit, also after an exception."""
    rec = _Record()
    original = ctx.alloc
    had_own = "alloc" in ctx.__dict__

    def alloc(n, ncols=1, dtype=np.float64, zero=True):
        block = original(n, ncols, dtype=dtype, zero=zero)
        if not zero:
            poison(block, value=value)
            rec.poisoned += 1
        rec.add(block)
        return block

    ctx.alloc = alloc
    try:
        yield rec
    finally:
        if had_own:
            ctx.alloc = original
        else:
            del ctx.alloc


def bits_equal(a, b, what="arrays"):
    """True when ``a`` and ``b`` have the same shape and the same raw 64-bit patterns (a NaN equals only the very same
    NaN, -0.0 differs from 0.0); otherwise an AssertionError that names the first position that differs."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s %s against %s %s" % (what, a.shape, a.dtype, b.shape, b.dtype)
    assert a.dtype in (np.dtype(np.float64), np.dtype(np.complex128)), "%s: %s is not a 64-bit float type" % (what, a.dtype)
    ua, ub = a.reshape(-1).view(np.uint64), b.reshape(-1).view(np.uint64)
    diff = np.flatnonzero(ua != ub)
    if diff.size:
        w = 2 if a.dtype.kind == "c" else 1
        i = int(diff[0])
        pos = np.unravel_index(i // w, a.shape) if a.ndim else ()
        fa, fb = a.reshape(-1).view(np.float64)[i], b.reshape(-1).view(np.float64)[i]
        raise AssertionError("%s: %d of %d words differ, first at %s%s: %r (%#018x) against %r (%#018x)" % (
            what, diff.size, ua.size, tuple(int(p) for p in pos), (" re", " im")[i % 2] if w == 2 else "",
            float(fa), int(ua[i]), float(fb), int(ub[i])))
    return True


def _apply_by_diagonals(A, x):
    """``A x`` in the type of ``x`` (longdouble / clongdouble), one diagonal of the sparse matrix after the other."""
    D = sp.dia_matrix(A)
    n = D.shape[0]
    y = np.zeros(n, dtype=x.dtype)
    for off, row in zip(D.offsets, D.data):
        off = int(off)
        # scipy's DIA layout: A[i, i + off] = row[i + off]
        i0, i1 = max(0, -off), min(n, D.shape[1] - off)
        if i1 > i0:
            y[i0:i1] += row[i0 + off: i1 + off].astype(x.dtype) * x[i0 + off: i1 + off]
    return y


def arnoldi_longdouble(A, v, m, sweeps, M_diag=None, lanczos=False):
    """``m`` Arnoldi steps from the start vector ``v`` in extended precision: operator, optional Lanczos pre-subtraction
    of ``h_{k,k-1} b_{k-1}``, modified Gram-Schmidt links left to right (``alpha = <v_j, w>``, ``h_jk += alpha``,
    ``w -= alpha b_j``) in ``sweeps`` passes, norm, division - with ``M_diag`` (a positive diagonal) the two-block form
    ``V = M P``, ``b_j = p_j``, norm ``sqrt(<w, M w>)``.  ``sweeps``: a number, or one number per step.  ``v`` is
    normalised here (for ``M_diag``: ``p_0 = v / sqrt(<v, M v>)``, ``v_0 = M p_0``).  Returns ``(H, V, P)`` as
    ``longdouble`` / ``clongdouble`` arrays (``P`` is None without ``M_diag``)."""
    cplx = np.iscomplexobj(v) or np.iscomplexobj(A.dtype.type(0))
    dt = np.clongdouble if cplx else np.longdouble
    n = v.shape[0]
    per_step = [int(sweeps)] * m if np.isscalar(sweeps) else [int(s) for s in sweeps]
    assert len(per_step) == m
    V = np.zeros((n, m + 1), dtype=dt, order="F")
    P = np.zeros((n, m + 1), dtype=dt, order="F") if M_diag is not None else None
    H = np.zeros((m + 1, m), dtype=dt)
    Md = None if M_diag is None else np.asarray(M_diag).astype(np.longdouble)
    x = np.asarray(v).reshape(-1).astype(dt)
    if Md is None:
        V[:, 0] = x / np.sqrt(np.vdot(x, x).real)
    else:
        P[:, 0] = x / np.sqrt(np.vdot(x, Md * x).real)
        V[:, 0] = Md * P[:, 0]
    B = V if Md is None else P
    for k in range(m):
        w = _apply_by_diagonals(A, V[:, k])
        start = 0
        if lanczos:
            start = k
            if k > 0:
                H[k - 1, k] = H[k, k - 1]
                w -= H[k, k - 1] * B[:, k - 1]
        for _ in range(per_step[k]):
            for j in range(start, k + 1):
                alpha = np.vdot(V[:, j], w)
                if lanczos:
                    alpha = alpha.real
                H[j, k] += alpha
                w -= alpha * B[:, j]
        if Md is None:
            H[k + 1, k] = np.sqrt(np.vdot(w, w).real)
            V[:, k + 1] = w / H[k + 1, k]
        else:
            Mw = Md * w
            H[k + 1, k] = np.sqrt(np.vdot(w, Mw).real)
            P[:, k + 1] = w / H[k + 1, k]
            V[:, k + 1] = Mw / H[k + 1, k]
    return H, V, P
