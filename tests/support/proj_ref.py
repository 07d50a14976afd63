"""The deflation projector in extended precision, and the comparison the tests of its device paths use - TEST
INFRASTRUCTURE ONLY, importable without a GPU.  Shares no code with ``krypy_amd``, ``oracle/`` or
``tests/support/numpy_context.py``.

``Projection.apply_complement`` as the deflated solvers run it (``kh_proj``): per sweep

    c = W[:, :d]^H z,    c' = T c  (``T is None``: c' = c),    z -= V[:, :d] c',

``iterations`` sweeps from ``z = a``, and ``ya = WRH c`` (``WRH is None``: ``c``) of the FIRST sweep.  ``W^H`` conjugates
``W``; ``T c`` and ``WRH c`` are plain matrix-vector products (no conjugate).

Every sum is ``(x * y).sum()``: NumPy's pairwise summation, in ``numpy.longdouble`` / ``numpy.clongdouble`` (64-bit
mantissa on x86) by default.  Columns of ``W`` and ``V`` are converted one at a time: no extended-precision copy of a block
is ever held.  The same code with ``dtype=numpy.float64`` is the ERROR YARDSTICK: what a straightforward float64
evaluation of the very same inputs loses against the extended one (``assert_matches``, the rule of
``tests/support/house_ref.py: step_bars`` with ``d`` in the floor)."""
import collections

import numpy as np

EPS = 2.2e-16

DeflatedStep = collections.namedtuple("DeflatedStep", "hcol ya v")


def _is_complex(*xs):
    return any(x is not None and np.iscomplexobj(x) for x in xs)


def _working_type(dtype, cplx):
    """The scalar type of a run: ``dtype`` names the precision (float64 / longdouble or their complex twins), ``cplx`` says
    whether the data are complex."""
    extended = np.dtype(dtype) in (np.dtype(np.longdouble), np.dtype(np.clongdouble))
    if cplx:
        return np.clongdouble if extended else np.complex128
    return np.longdouble if extended else np.float64


def _sum(x, y):
    return (x * y).sum()


def _small(M, dt):
    return None if M is None else np.array(M, dtype=dt)


def _sweeps(W, V, d, T, WRH, iterations, z, dt):
    """The sweeps on ``z`` (in place, already of type ``dt``); returns ``ya`` of the first one."""
    T, WRH = _small(T, dt), _small(WRH, dt)
    ya = None
    for it in range(int(iterations)):
        c = np.zeros(d, dtype=dt)
        for j in range(d):
            w = np.asarray(W[:, j]).astype(dt, copy=False)
            c[j] = _sum(np.conj(w), z)
        if it == 0:
            ya = c.copy() if WRH is None else np.array([_sum(WRH[i, :d], c) for i in range(d)], dtype=dt)
        cp = c if T is None else np.array([_sum(T[i, :d], c) for i in range(d)], dtype=dt)
        for j in range(d):
            v = np.asarray(V[:, j]).astype(dt, copy=False)
            z -= cp[j] * v
    return ya


def complement(W, V, d, T, WRH, iterations, a, dtype=np.longdouble):
    """``(z, ya)`` of the module docstring.  ``W``, ``V``: ``(n, >= d)`` arrays (only columns ``0 .. d-1`` are read), ``T``,
    ``WRH``: ``(d, d)`` or ``None``, ``a``: the vector.  Real and complex inputs; the result has the precision of ``dtype``."""
    d = int(d)
    assert d >= 1 and iterations >= 1
    dt = _working_type(dtype, _is_complex(W, V, T, WRH, a))
    z = np.array(np.asarray(a).reshape(-1), dtype=dt)
    ya = _sweeps(W, V, d, T, WRH, iterations, z, dt)
    return z, ya


def deflated_step(A, W, V, d, T, WRH, iterations, Vbasis, k, sweeps, dtype=np.longdouble):
    """One deflated Arnoldi step: ``w = A v_k`` (the SciPy / NumPy product in working precision - float64 or complex128 -, as
    the device's SpMV is bit-identical to it), the projection above on ``w``, ``sweeps`` passes of modified Gram-Schmidt
    against columns ``0 .. k`` of ``Vbasis`` (coefficients of the passes added up), the norm and ``v_{k+1}``.
    Returns ``DeflatedStep(hcol[k + 2], ya[d], v)``: ``hcol[k + 1]`` is the norm."""
    k = int(k)
    Vbasis = np.asarray(Vbasis)
    w = np.asarray(A.dot(Vbasis[:, k])).reshape(-1)
    dt = _working_type(dtype, _is_complex(W, V, T, WRH, w, Vbasis))
    z = np.array(w, dtype=dt)
    ya = _sweeps(W, V, int(d), T, WRH, iterations, z, dt)
    hcol = np.zeros(k + 2, dtype=dt)
    for _ in range(int(sweeps)):
        for j in range(k + 1):
            v = Vbasis[:, j].astype(dt, copy=False)
            h = _sum(np.conj(v), z)
            z -= h * v
            hcol[j] += h
    nrm = np.sqrt(_sum(np.conj(z), z).real)
    hcol[k + 1] = nrm
    return DeflatedStep(hcol, ya, z / nrm)


def _quantities(x):
    """``{name: array}`` of a result: a ``DeflatedStep``, a ``(z, ya)`` pair or a dict; a ``ya`` of ``None`` is left out."""
    if isinstance(x, dict):
        q = dict(x)
    elif hasattr(x, "_fields"):
        q = dict(zip(x._fields, x))
    else:
        z, ya = x
        q = {"z": z, "ya": ya}
    return {n: np.asarray(v).reshape(-1) for n, v in q.items() if v is not None}


def _norm(x):
    x = np.asarray(x)
    return np.sqrt((x * np.conj(x)).real.sum())


def errors(got, ref, scale):
    """The error of each quantity ``got`` holds against ``ref``: ``z`` as the 2-norm of the difference over ``scale``
    (``||a||``), ``ya`` and ``hcol`` over the 2-norm of the reference (over ``scale`` where that is zero), ``v`` - a unit
    vector - as the 2-norm of the difference."""
    got, ref = _quantities(got), _quantities(ref)
    wide = np.clongdouble
    out = {}
    for name, g in got.items():
        if name not in ref:
            raise AssertionError("%s returned, the reference has none" % name)
        r = ref[name]
        if g.shape != r.shape:
            raise AssertionError("%s: shape %s, expected %s" % (name, g.shape, r.shape))
        diff = _norm(g.astype(wide) - r.astype(wide))
        if name == "z":
            den = np.longdouble(scale)
        elif name == "v":
            den = np.longdouble(1)
        else:
            den = _norm(r.astype(wide))
            if den == 0:
                den = np.longdouble(scale)
        out[name] = float(diff / den)
    return out


def bars(ref, yardstick, d, scale):
    """``16 x max(E64, eps sqrt(d + 1))`` per quantity: ``E64`` is the same error of the float64 run of the reference on the
    same inputs, the factor 16 covers another order of summation.  Returns ``(bars, e64)``."""
    e64 = errors(yardstick, ref, scale)
    floor = EPS * np.sqrt(d + 1.0)
    return {q: 16.0 * max(e, floor) for q, e in e64.items()}, e64


def assert_matches(got, ref, yardstick, d, scale):
    """The comparison of the projector tests.  ``got``, ``ref``, ``yardstick``: ``(z, ya)`` pairs or ``DeflatedStep``
    tuples (``ref`` in extended precision, ``yardstick`` its float64 run on the same inputs); a ``ya`` of ``None`` in ``got``
    (not requested) is not compared.  Every quantity within its bar (``bars``).  Returns ``(errors, bars)``; raises an
    AssertionError that names the quantity otherwise (a NaN fails)."""
    errs = errors(got, ref, scale)
    bar, _ = bars(ref, yardstick, d, scale)
    if not errs:
        raise AssertionError("nothing to compare")
    for q in sorted(errs):
        if not errs[q] <= bar[q]:
            raise AssertionError("d = %d: %s is off by %.3e, the bar is %.3e" % (d, q, errs[q], bar[q]))
    return errs, {q: bar[q] for q in errs}
