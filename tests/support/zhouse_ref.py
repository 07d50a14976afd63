"""The complex Householder Arnoldi step in extended precision, and the comparison the GPU tests of ``k_zhouse_chain`` use -
TEST INFRASTRUCTURE ONLY, importable without a GPU.  Shares no code with ``krypy_amd`` or ``oracle/``.

One step ``k`` from given inputs (complex reflector columns ``u_0 .. u_k``, zero above their own row, their REAL factors
``beta_j``, and ``w = A v_k``), in the form the one-launch kernel (``krypy_amd/csrc/house.h``, ``k_zhouse_chain``) computes it:

* forward links ``j = 0 .. k``: ``d = conj(u_j) . w``, ``w -= (beta_j d) u_j``; a link with ``beta_j == 0`` is skipped; the
  factors ``conj(alpha_j)`` are NOT applied (the host applies them to the rows it gets back);
* ``gamma = w[k+1]`` (complex), ``sigma^2 = sum_{i > k+1} |w_i|^2`` (real), and from them ``(v0, xnorm, alpha, beta)`` with the
  branches of the reference's ``House`` for a complex ``gamma`` (no row behind ``k+1`` or ``sigma == 0``: ``v0 = 1``,
  ``xnorm = |gamma|``, ``beta = 0``, ``alpha = gamma / |gamma|`` or 1; else ``xnorm = sqrt(|gamma|^2 + sigma^2)``, ``beta = 2`` and
  ``v0 = -sigma``, ``alpha = 1`` for ``gamma == 0``, ``v0 = gamma + gamma / |gamma| xnorm``, ``alpha = -gamma / |gamma|`` otherwise);
* ``u_{k+1} = [0 .. 0, v0, w_{k+2:}] / sqrt(|v0|^2 + sigma^2)``;
* ``x = e_{k+1} - beta conj(u_{k+1}[k+1]) u_{k+1}`` (the coefficient is ``u_{k+1}^* e_{k+1}``), backward links ``j = k .. 0`` on
  ``x``, ``v_{k+1} = alpha x``.

Every sum is ``(a * b).sum()``: NumPy's pairwise summation, in ``numpy.clongdouble`` (64-bit mantissas on x86) by default.
The same code with ``dtype=numpy.complex128`` is the ERROR YARDSTICK of the GPU tests: what a straightforward complex128
evaluation of the very same inputs loses against the extended-precision one (``assert_zstep_matches``)."""
import collections

import numpy as np

EPS = 2.2e-16

ZStep = collections.namedtuple("ZStep", "raw gamma sigma2 xnorm alpha beta u v")

QUANTITIES = ("raw", "gamma", "sigma2", "xnorm", "alpha", "u", "v")


def crel(a, b):
    """``||a - b|| / ||b||`` of complex arrays (``tests.parity_cases.rel`` keeps the real parts only)."""
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300)


def _real_type(dtype):
    return np.longdouble if np.dtype(dtype) == np.dtype(np.clongdouble) else np.float64


def _cdot(u, w):
    return (np.conj(u) * w).sum()


def zhouse_step_longdouble(columns, beta, w, k, dtype=np.clongdouble):
    """One step (module docstring).  ``columns``: a callable ``j -> complex128 column``, ``beta``: the real factors
    ``beta_0 .. beta_k``, ``w``: ``A v_k``, ``k >= -1`` (``-1``: no link, reflector 0 from ``w`` itself).  Returns
    ``ZStep(raw[0..k], gamma, sigma2, xnorm, alpha, beta, u, v)`` in ``dtype`` (``sigma2``, ``xnorm``, ``beta`` real)."""
    ct = np.dtype(dtype).type
    rt = _real_type(dtype)
    w = np.array(w, dtype=ct).reshape(-1)
    n = w.shape[0]
    assert -1 <= k and k + 1 < n
    b = [float(beta[j]) for j in range(k + 1)]
    for j in range(k + 1):
        if b[j] != 0.0:
            u = np.asarray(columns(j)).reshape(-1).astype(ct, copy=False)
            w -= (rt(b[j]) * _cdot(u, w)) * u
    raw = w[: k + 1].copy()
    gamma = w[k + 1]
    tail = w[k + 2:]
    sigma2 = (tail.real * tail.real + tail.imag * tail.imag).sum() if tail.size else rt(0)
    sigma = np.sqrt(sigma2)
    ag = np.abs(gamma)
    if sigma == 0:
        v0, xnorm, bnew = ct(1), ag, rt(0)
        alpha = ct(1) if gamma == 0 else gamma / ag
    else:
        xnorm, bnew = np.sqrt(ag * ag + sigma * sigma), rt(2)
        if gamma == 0:
            v0, alpha = ct(-sigma), ct(1)
        else:
            sg = gamma / ag
            v0, alpha = gamma + sg * xnorm, -sg
    unew = np.zeros(n, dtype=ct)
    unew[k + 1] = v0
    unew[k + 2:] = tail
    unew /= np.sqrt(np.abs(v0) ** 2 + sigma * sigma)
    x = np.zeros(n, dtype=ct)
    x[k + 1] = 1
    x -= (bnew * np.conj(unew[k + 1])) * unew
    for j in range(k, -1, -1):
        if b[j] != 0.0:
            u = np.asarray(columns(j)).reshape(-1).astype(ct, copy=False)
            x -= (rt(b[j]) * _cdot(u, x)) * u
    return ZStep(raw, gamma, sigma2, xnorm, alpha, bnew, unew, alpha * x)


class ZReflectorState(object):
    """Seeded complex reflector columns: column ``j`` is a random complex unit vector that is zero above row ``j``, its factor
    is 2.0 - a genuine reflector - except at the indices in ``zero_beta`` (factor 0.0: the identity, its column is still
    random, so a link that is wrongly NOT skipped shows).  Any column can be made again from the seed."""

    def __init__(self, n, ncols, seed, zero_beta=()):
        self.n, self.ncols, self.seed = int(n), int(ncols), int(seed)
        assert self.ncols <= self.n
        self.beta = np.full(self.ncols, 2.0)
        for j in zero_beta:
            self.beta[j] = 0.0

    def column(self, j):
        rng = np.random.default_rng([self.seed, j])
        x = (rng.random(self.n - j) - 0.5) + 1j * (rng.random(self.n - j) - 0.5)
        if abs(x[0]) < 1e-3:          # (a single-entry column must not vanish)
            x[0] = 0.25 - 0.125j
        c = np.zeros(self.n, dtype=np.complex128)
        c[j:] = x / np.sqrt(np.vdot(x, x).real)
        return c

    def block(self, j0, j1):
        out = np.zeros((self.n, j1 - j0), dtype=np.complex128, order="F")
        for j in range(j0, j1):
            out[:, j - j0] = self.column(j)
        return out


def _as_step(x):
    return x if isinstance(x, ZStep) else ZStep(*x)


def zstep_errors(got, ref, wnorm):
    """The error of each quantity of one step against the reference: ``raw`` and ``gamma`` as max-abs (of the complex
    difference) over ``||w||``, ``sigma2`` and ``xnorm`` relative, ``alpha`` absolute (``|alpha| = 1``), ``u`` and ``v`` as
    the 2-norm of the difference (both are unit vectors).  ``gamma`` / ``sigma2`` of ``got`` may be None (the per-reflector
    path does not keep them): they are left out."""
    got, ref = _as_step(got), _as_step(ref)
    ld, cld = np.longdouble, np.clongdouble
    out = {}
    graw, rraw = np.asarray(got.raw, dtype=cld), np.asarray(ref.raw, dtype=cld)
    if graw.shape != rraw.shape:
        raise AssertionError("raw rows: %d returned, %d expected" % (graw.size, rraw.size))
    out["raw"] = float(np.max(np.abs(graw - rraw)) / ld(wnorm)) if rraw.size else 0.0
    if got.gamma is not None:
        out["gamma"] = float(np.abs(cld(got.gamma) - cld(ref.gamma)) / ld(wnorm))
    for name in ("sigma2", "xnorm"):
        if getattr(got, name) is None:
            continue
        g, r = ld(np.real(getattr(got, name))), ld(np.real(getattr(ref, name)))
        out[name] = float(abs(g - r) / abs(r)) if r != 0 else (0.0 if g == 0 else float("inf"))
    out["alpha"] = float(np.abs(cld(got.alpha) - cld(ref.alpha)))
    for name in ("u", "v"):
        g, r = np.asarray(getattr(got, name)), np.asarray(getattr(ref, name))
        if g.shape != r.shape:
            raise AssertionError("%s: shape %s, expected %s" % (name, g.shape, r.shape))
        d = g.astype(cld) - r
        out[name] = float(np.sqrt((d.real * d.real + d.imag * d.imag).sum()))
    return out


def zstep_bars(ref, yardstick, k, wnorm):
    """``16 x max(E64, eps sqrt(k+2))`` per quantity: ``E64`` is the same error of the complex128 run of the step reference
    on the same inputs, the factor 16 covers another order of summation."""
    e64 = zstep_errors(yardstick, ref, wnorm)
    floor = EPS * np.sqrt(k + 2.0)
    return {q: 16.0 * max(e, floor) for q, e in e64.items()}, e64


def assert_zstep_matches(got, ref, yardstick, k, wnorm):
    """The comparison of the GPU tests.  ``got``, ``ref``, ``yardstick``: ``ZStep`` tuples (``ref`` in extended precision,
    ``yardstick`` its complex128 run).  Every quantity within its bar (``zstep_bars``), ``beta`` exactly the reference's,
    ``sigma2`` / ``xnorm`` / ``beta`` real, rows ``0 .. k`` of the new reflector exactly ``+0.0`` in both parts.  Returns
    ``(errors, bars)``; raises an AssertionError that names the quantity otherwise (a NaN fails)."""
    got, ref = _as_step(got), _as_step(ref)
    errs = zstep_errors(got, ref, wnorm)
    bars, _ = zstep_bars(ref, yardstick, k, wnorm)
    for q in QUANTITIES:
        if q not in errs:          # (gamma / sigma2 of a step re-run per reflector)
            continue
        if not errs[q] <= bars[q]:
            raise AssertionError("step k = %d: %s is off by %.3e, the bar is %.3e" % (k, q, errs[q], bars[q]))
    for name in ("sigma2", "xnorm", "beta"):
        if getattr(got, name) is not None and np.imag(getattr(got, name)) != 0:
            raise AssertionError("step k = %d: %s = %r is not real" % (k, name, getattr(got, name)))
    if not float(np.real(got.beta)) == float(ref.beta):
        raise AssertionError("step k = %d: beta = %r, the reference has %r" % (k, got.beta, float(ref.beta)))
    head = np.ascontiguousarray(np.asarray(got.u, dtype=np.complex128)[: k + 1])
    bad = np.flatnonzero(head.view(np.uint64))
    if bad.size:
        raise AssertionError("step k = %d: word %d of the new reflector's head is not +0.0 (%d such words above row %d)" % (
            k, int(bad[0]), bad.size, k + 1))
    return errs, bars
