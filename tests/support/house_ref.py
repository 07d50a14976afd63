"""The Householder Arnoldi step in extended precision, and the comparison the GPU tests of ``k_house_chain`` use -
TEST INFRASTRUCTURE ONLY, importable without a GPU.  Shares no code with ``krypy_amd`` or ``oracle/``.

One step ``k`` from given inputs (reflector columns ``u_0 .. u_k``, zero above their own row, their factors ``beta_j``, and
``w = A v_k``), in the form the one-launch kernel (``krypy_amd/csrc/house.h``) computes it:

* forward links ``j = 0 .. k``: ``d = <u_j, w>``, ``w -= (beta_j d) u_j``; a link with ``beta_j == 0`` is skipped; the factors
  ``conj(alpha_j)`` are NOT applied (the host applies them to the rows it gets back);
* ``gamma = w[k+1]``, ``sigma^2 = sum_{i > k+1} w_i^2``, and from them ``(v0, xnorm, alpha, beta)`` with the branches of the
  reference's ``House`` (no row behind ``k+1`` or ``sigma == 0``: ``v0 = 1``, ``xnorm = |gamma|``, ``beta = 0``,
  ``alpha = gamma / |gamma|`` or 1; else ``xnorm = sqrt(gamma^2 + sigma^2)``, ``beta = 2`` and ``v0 = -sigma``, ``alpha = 1`` for
  ``gamma == 0``, ``v0 = gamma + sign(gamma) xnorm``, ``alpha = -sign(gamma)`` otherwise);
* ``u_{k+1} = [0 .. 0, v0, w_{k+2:}] / sqrt(v0^2 + sigma^2)``;
* ``x = e_{k+1} - beta u_{k+1}[k+1] u_{k+1}``, backward links ``j = k .. 0`` on ``x``, ``v_{k+1} = alpha x``.

Every sum is ``(a * b).sum()``: NumPy's pairwise summation, in ``numpy.longdouble`` (64-bit mantissa on x86) by default.  The
same code with ``dtype=numpy.float64`` is the ERROR YARDSTICK of the GPU tests: what a straightforward float64 evaluation of
the very same inputs loses against the extended-precision one (``assert_step_matches``)."""
import collections

import numpy as np

from tests.support.poison import _apply_by_diagonals

EPS = 2.2e-16

Step = collections.namedtuple("Step", "raw gamma sigma2 xnorm alpha beta u v")


def _sum(a, b):
    return (a * b).sum()


def house_step_longdouble(columns, beta, w, k, dtype=np.longdouble):
    """One step (module docstring).  ``columns``: a callable ``j -> float64 column`` (converted one at a time: no extended
    copy of the block is ever held), ``beta``: the factors ``beta_0 .. beta_k``, ``w``: ``A v_k``, ``k >= -1`` (``-1``: no
    link, reflector 0 from ``w`` itself).  Returns ``Step(raw[0..k], gamma, sigma2, xnorm, alpha, beta, u, v)`` in ``dtype``."""
    dt = np.dtype(dtype).type
    w = np.array(w, dtype=dt).reshape(-1)
    n = w.shape[0]
    assert -1 <= k and k + 1 < n
    b = [float(beta[j]) for j in range(k + 1)]
    for j in range(k + 1):
        if b[j] != 0.0:
            u = np.asarray(columns(j)).reshape(-1).astype(dt, copy=False)
            w -= (dt(b[j]) * _sum(u, w)) * u
    raw = w[: k + 1].copy()
    gamma = w[k + 1]
    tail = w[k + 2:]
    sigma2 = _sum(tail, tail) if tail.size else dt(0)
    sigma = np.sqrt(sigma2)
    if sigma == 0:
        v0, xnorm, bnew = dt(1), abs(gamma), dt(0)
        alpha = dt(1) if gamma == 0 else gamma / xnorm
    else:
        xnorm, bnew = np.sqrt(gamma * gamma + sigma * sigma), dt(2)
        if gamma == 0:
            v0, alpha = -sigma, dt(1)
        else:
            sg = gamma / abs(gamma)
            v0, alpha = gamma + sg * xnorm, -sg
    unew = np.zeros(n, dtype=dt)
    unew[k + 1] = v0
    unew[k + 2:] = tail
    unew /= np.sqrt(v0 * v0 + sigma * sigma)
    x = np.zeros(n, dtype=dt)
    x[k + 1] = 1
    x -= (bnew * unew[k + 1]) * unew
    for j in range(k, -1, -1):
        if b[j] != 0.0:
            u = np.asarray(columns(j)).reshape(-1).astype(dt, copy=False)
            x -= (dt(b[j]) * _sum(u, x)) * u
    return Step(raw, gamma, sigma2, xnorm, alpha, bnew, unew, alpha * x)


def house_arnoldi_longdouble(A, v, m, dtype=np.longdouble):
    """``m`` Householder Arnoldi steps from the start vector ``v``, built on the step: reflector 0 comes from ``v`` as a step
    with ``k = -1``, ``H[:k+1, k] = raw * alpha[:k+1]``, ``H[k+1, k] = xnorm``.  Returns ``(H, V, U, alpha, beta)`` in
    ``dtype`` (``U``: the reflector block)."""
    dt = np.dtype(dtype).type
    n = np.asarray(v).reshape(-1).shape[0]
    U = np.zeros((n, m + 1), dtype=dt, order="F")
    V = np.zeros((n, m + 1), dtype=dt, order="F")
    H = np.zeros((m + 1, m), dtype=dt)
    alpha, beta = np.zeros(m + 1, dtype=dt), np.zeros(m + 1)
    cols = lambda j: U[:, j]            # noqa: E731
    s = house_step_longdouble(cols, beta, np.asarray(v).reshape(-1), -1, dtype)
    U[:, 0], V[:, 0], alpha[0], beta[0] = s.u, s.v, s.alpha, float(s.beta)
    for k in range(m):
        s = house_step_longdouble(cols, beta, _apply_by_diagonals(A, V[:, k]), k, dtype)
        H[: k + 1, k] = s.raw * alpha[: k + 1]
        H[k + 1, k] = s.xnorm
        U[:, k + 1], V[:, k + 1], alpha[k + 1], beta[k + 1] = s.u, s.v, s.alpha, float(s.beta)
    return H, V, U, alpha, beta


class ReflectorState(object):
    """Seeded reflector columns: column ``j`` is a random unit vector that is zero above row ``j``, its factor is 2.0 -
    a genuine reflector - except at the indices in ``zero_beta`` (factor 0.0: the identity, its column is still random, so a
    link that is wrongly NOT skipped shows).  Any column can be made again from the seed."""

    def __init__(self, n, ncols, seed, zero_beta=()):
        self.n, self.ncols, self.seed = int(n), int(ncols), int(seed)
        assert self.ncols <= self.n
        self.beta = np.full(self.ncols, 2.0)
        for j in zero_beta:
            self.beta[j] = 0.0

    def column(self, j):
        x = np.random.default_rng([self.seed, j]).random(self.n - j) - 0.5
        if abs(x[0]) < 1e-3:          # (a single-entry column must not vanish)
            x[0] = 0.25
        c = np.zeros(self.n)
        c[j:] = x / np.sqrt(np.dot(x, x))
        return c

    def block(self, j0, j1):
        out = np.zeros((self.n, j1 - j0), order="F")
        for j in range(j0, j1):
            out[:, j - j0] = self.column(j)
        return out


def reflector_state(n, ncols, seed, zero_beta=()):
    return ReflectorState(n, ncols, seed, zero_beta)


def _as_step(x):
    return x if isinstance(x, Step) else Step(*x)


def step_errors(got, ref, wnorm):
    """The error of each quantity of one step against the reference: ``raw`` and ``gamma`` as max-abs over ``||w||``,
    ``sigma2`` and ``xnorm`` relative, ``u`` and ``v`` as the 2-norm of the difference (both are unit vectors)."""
    got, ref = _as_step(got), _as_step(ref)
    ld = np.longdouble
    out = {}
    graw, rraw = np.asarray(got.raw, dtype=ld), np.asarray(ref.raw, dtype=ld)
    if graw.shape != rraw.shape:
        raise AssertionError("raw rows: %d returned, %d expected" % (graw.size, rraw.size))
    out["raw"] = float(np.max(np.abs(graw - rraw)) / ld(wnorm)) if rraw.size else 0.0
    out["gamma"] = float(abs(ld(got.gamma) - ld(ref.gamma)) / ld(wnorm))
    for name in ("sigma2", "xnorm"):
        g, r = ld(getattr(got, name)), ld(getattr(ref, name))
        out[name] = float(abs(g - r) / abs(r)) if r != 0 else (0.0 if g == 0 else float("inf"))
    for name in ("u", "v"):
        g, r = np.asarray(getattr(got, name)), np.asarray(getattr(ref, name))
        if g.shape != r.shape:
            raise AssertionError("%s: shape %s, expected %s" % (name, g.shape, r.shape))
        d = g.astype(ld) - r
        out[name] = float(np.sqrt((d * d).sum()))
    return out


def step_bars(ref, yardstick, k, wnorm):
    """``16 x max(E64, eps sqrt(k+2))`` per quantity: ``E64`` is the same error of the float64 run of the step reference on
    the same inputs, the factor 16 covers another order of summation."""
    e64 = step_errors(yardstick, ref, wnorm)
    floor = EPS * np.sqrt(k + 2.0)
    return {q: 16.0 * max(e, floor) for q, e in e64.items()}, e64


def assert_step_matches(got, ref, yardstick, k, wnorm):
    """The comparison of the GPU tests.  ``got``, ``ref``, ``yardstick``: ``Step`` tuples (``ref`` in extended precision,
    ``yardstick`` its float64 run).  Every quantity within its bar (``step_bars``), ``alpha`` and ``beta`` exactly the
    reference's, rows ``0 .. k`` of the new reflector exactly ``+0.0``.  Returns ``(errors, bars)``; raises an
    AssertionError that names the quantity otherwise (a NaN fails)."""
    got, ref = _as_step(got), _as_step(ref)
    errs = step_errors(got, ref, wnorm)
    bars, _ = step_bars(ref, yardstick, k, wnorm)
    for q in ("raw", "gamma", "sigma2", "xnorm", "u", "v"):
        if not errs[q] <= bars[q]:
            raise AssertionError("step k = %d: %s is off by %.3e, the bar is %.3e" % (k, q, errs[q], bars[q]))
    if not float(got.alpha) == float(ref.alpha):
        raise AssertionError("step k = %d: alpha = %r, the reference has %r" % (k, float(got.alpha), float(ref.alpha)))
    if not float(got.beta) == float(ref.beta):
        raise AssertionError("step k = %d: beta = %r, the reference has %r" % (k, float(got.beta), float(ref.beta)))
    head = np.ascontiguousarray(np.asarray(got.u, dtype=np.float64)[: k + 1])
    bad = np.flatnonzero(head.view(np.uint64))
    if bad.size:
        raise AssertionError("step k = %d: row %d of the new reflector is %r, not +0.0 (%d such rows above row %d)" % (
            k, int(bad[0]), float(head[bad[0]]), bad.size, k + 1))
    return errs, bars
