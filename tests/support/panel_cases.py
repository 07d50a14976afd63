"""The catalogue of tests/test_gpu_panel.py: which widths, row counts and pass counts are run, and WHY - every case names the
edges of the host code it selects, as predicates over the split plans of tests/support/panel_ref.py.  tests/test_panel_host.py
holds every predicate on the CPU; the data generators are here too, so that both files see the same numbers."""
import collections

import numpy as np

from tests.support import panel_ref as pr

REAL_WIDTHS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 47, 1023, 1024, 1025)
C128_WIDTHS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 511, 512, 513)
ROWS = (1, 2, 3, 255, 256, 257, 511, 513, 4097, 100003)
WIDE_FROM, WIDE_ROWS = 511, 257           # the widths from 511 up run at 257 rows only
GRIDS = (0, 1, 3)                         # reduce_blocks: the default, and two at which the grid-stride loops make several trips
GEMM_K = (0, 1, 16, 17, 1023, 1024, 1025, 2049)
GEMM_AB = ((1.0, 0.0), (1.0, 1.0), (-0.75, 1.0), (2.0, 0.5), (0.0, 0.5))
GEMM_NC = (1, 17, 20)                     # per-column form by shape; 2 ... 16 take it with gram_mfma off
GEMM_NC_OFF = (2, 16)
MFMA_K = (1024, 1025, 1100)
MFMA_NC = (2, 16)
ZGEMM_K = (0, 1, 8, 9, 511, 512, 513, 1025)
ZGEMM_BETA = (0.0, 1.0, 0.5)
TAIL_COLS = (1, 2, 3, 16, 17, 33)         # k + 1 of the Arnoldi step that reaches the fused tails


# ---- predicates: name -> (path, width) -> bool -------------------------------------------------------------------------------
def _split(path, w):
    return pr.split_real(w) if path == "real" else pr.split_c128(w)


def _cap(path):
    return pr.CAP if path == "real" else pr.ZCAP


def _first_call(path, w):
    return min(w, _cap(path))


EDGES = collections.OrderedDict([
    ("one launch", lambda p, w: len(_split(p, _first_call(p, w))) == 1),
    ("second chunk: coef_dev + done, later chunks keep w", lambda p, w: len(_split(p, _first_call(p, w))) >= 2),
    ("last chunk is a single column", lambda p, w: len(_split(p, w)) >= 2 and _split(p, w)[-1] == 1),
    ("every chunk size in one call", lambda p, w: sorted(set(_split(p, w))) == ([1, 2, 4, 8, 16] if p == "real" else [1, 2, 4, 8])),
    ("the widest launch twice", lambda p, w: _split(p, w)[:2] == [pr.MAXC if p == "real" else pr.ZMAXC] * 2),
    ("second outer chunk of dot_panel_dev: out_dev + done", lambda p, w: p == "real" and len(pr.outer_chunks(_first_call(p, w))) >= 2),
    ("outer chunk of one column", lambda p, w: p == "real" and pr.outer_chunks(_first_call(p, w))[-1] == 1 and w > 1),
    ("one below the cap", lambda p, w: w == _cap(p) - 1),
    ("exactly at the cap: the coefficients fill SC_COEF ... SC_LS", lambda p, w: w == _cap(p)),
    ("wrapper splits: a second C call of one column", lambda p, w: pr.wrapper_calls(w, _cap(p)) == [_cap(p), 1]),
])

Case = collections.namedtuple("Case", "path width rows edges")


def _rows_for(width):
    return (WIDE_ROWS,) if width >= WIDE_FROM else ROWS


def _claimed(path, width):
    return tuple(name for name, f in EDGES.items() if f(path, width))


CASES = tuple(Case(p, w, _rows_for(w), _claimed(p, w)) for p, ws in (("real", REAL_WIDTHS), ("c128", C128_WIDTHS)) for w in ws)

# what the catalogue as a whole must reach (tests/test_panel_host.py): every edge, on the path it exists on
REQUIRED = {
    "real": tuple(EDGES),
    "c128": tuple(n for n in EDGES if "dot_panel_dev" not in n and "outer chunk" not in n),
}

# the pass edges of kh_gemm_nn (real: passes of KMAX inside the C call; c128: calls of ZCAP from the wrapper; MFMA: passes of 64)
K_EDGES = collections.OrderedDict([
    ("k == 0: no column, Y scaled", lambda k, per: k == 0),
    ("one column", lambda k, per: k == 1),
    ("inside one pass", lambda k, per: 1 < k < per - 1),
    ("one below a full pass", lambda k, per: k == per - 1),
    ("exactly one full pass", lambda k, per: k == per),
    ("second pass of one column: it starts from 1, not from beta", lambda k, per: pr.passes(k, per) == [per, 1]),
    ("third pass", lambda k, per: len(pr.passes(k, per)) == 3),
])


def k_edges(k, per):
    return tuple(name for name, f in K_EDGES.items() if f(k, per))


def narrow(widths):
    return tuple(w for w in widths if w < WIDE_FROM)


def wide(widths):
    return tuple(w for w in widths if w >= WIDE_FROM)


def offsets(width, ncols):
    """The column offsets a width is run at inside a block of ``ncols`` data columns: 1, and flush with the block's end."""
    return tuple(sorted({1, ncols - width}))


# ---- data ----------------------------------------------------------------------------------------------------------------------
def col_scale(j):
    """Every column has its own scale (a swapped slot, a coefficient of the wrong chunk moves the result): a power of two from
    1/4 to 4 times an odd fraction in [1, 2)."""
    j = np.asarray(j)
    return 2.0 ** ((j % 5) - 2) * (1.0 + (2 * (j % 127) + 1) / 256.0)


def block(n, ncols, seed, cplx=False):
    """(n, ncols) with magnitudes in [1, 2) times the column's scale and random signs: no cancellation inside a product, a lost
    or repeated term moves a sum by at least a quarter.  Complex: the imaginary part has its own magnitudes, signs and a
    different scale (0.625 of the real part's), so that conj(v) w, v w and v conj(w) all differ."""
    rng = np.random.default_rng(seed)

    def part():
        return (1.0 + rng.random((n, ncols))) * rng.choice([-1.0, 1.0], size=(n, ncols))

    s = col_scale(np.arange(ncols))[None, :]
    if not cplx:
        return np.asfortranarray(part() * s)
    return np.asfortranarray(part() * s + 1j * (part() * (0.625 * s)))


def coefficients(k, seed, cplx=False):
    """k distinct coefficients with magnitudes in [1/2, 3/2) and random signs."""
    rng = np.random.default_rng(seed)

    def part():
        return (0.5 + rng.random(k)) * rng.choice([-1.0, 1.0], size=k)

    return part() + 1j * (0.75 * part()) if cplx else part()
