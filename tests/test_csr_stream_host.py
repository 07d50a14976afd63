"""CPU tests of the catalogue behind tests/test_gpu_csr_stream.py (tests/support/csr_stream_cases.py): every structure selects
the path it claims, the plan replica follows the greedy rule stated by brute force, and the partial-sum slots of the widest
reduction grid fit the allocation - read from the sources, so that a changed constant fails here."""
import os
import re

import numpy as np
import pytest

from tests.support import csr_stream_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krypy_amd", "csrc")


@pytest.mark.parametrize("T", cs.TILES)
@pytest.mark.parametrize("name", sorted(cs.REAL))
def test_every_structure_selects_what_it_claims(name, T):
    c = cs.case(name, T)
    p = cs.window_plan(c.A, T)
    assert c.holds(p), "%r: %s\nfit %d of %d, widest %d, window %s" % (c, c.claim, p["fit"], p["nblk"], p["widest"],
                                                                       p["window_on"])
    A = c.A
    assert A.has_sorted_indices and A.shape[0] <= 25000
    lens = np.diff(A.indptr)
    rows = np.repeat(np.arange(A.shape[0]), lens)
    assert np.all(np.diff(A.indices)[np.diff(rows) == 0] > 0), "columns ascend strictly within every row"
    assert np.all(A.data != 0.0)
    if name != "banded_on_stream":
        assert np.all((np.abs(A.data) >= 1.0) & (np.abs(A.data) < 2.0)) and (A.data < 0).any() and (A.data > 0).any()
    assert np.array_equal(c.long_rows, np.nonzero(lens > T)[0])


@pytest.mark.parametrize("T", cs.ZTILES)
@pytest.mark.parametrize("name", sorted(cs.COMPLEX))
def test_complex_twins_keep_the_pattern_and_the_claim(name, T):
    z, c = cs.zcase(name, T), cs.case(name, T)
    assert z.A.dtype == np.complex128 and z.holds(cs.window_plan(z.A, T))
    assert np.array_equal(z.A.indptr, c.A.indptr) and np.array_equal(z.A.indices, c.A.indices)
    for part in (z.A.data.real, z.A.data.imag):
        assert np.all((np.abs(part) >= 1.0) & (np.abs(part) < 2.0)) and (part < 0).any() and (part > 0).any()


@pytest.mark.parametrize("T", cs.TILES)
def test_widening_does_not_move_block_borders(T):
    base = cs.rowblocks(cs.case("all_fit", T).A.indptr, T)
    assert base.size == 41
    for name in ("nine_of_ten", "below_nine_of_ten", "span_4096", "span_4097"):
        assert np.array_equal(cs.rowblocks(cs.case(name, T).A.indptr, T), base), name


def test_the_threshold_is_nine_blocks_in_ten():
    """36 of 40 is on, 35 of 40 is off, and the same two matrices differ in ONE entry's column."""
    for T in cs.TILES:
        on, off = cs.case("nine_of_ten", T), cs.case("below_nine_of_ten", T)
        assert on.plan["window_on"] and not off.plan["window_on"]
        assert (on.plan["fit"], off.plan["fit"]) == (36, 35)
        assert np.array_equal(on.A.indptr, off.A.indptr) and np.count_nonzero(on.A.indices != off.A.indices) == 1


def _brute_force_blocks(lens, tile):
    """The rule stated block by block: a block is the LONGEST run of rows from its first one that has at most 1024 rows and at
    most ``tile`` entries - and one row where no such run exists."""
    n = len(lens)
    upto = [0]
    for v in lens:
        upto.append(upto[-1] + int(v))
    out = [0]
    while out[-1] < n:
        r = out[-1]
        ok = [e for e in range(r + 1, min(n, r + cs.MAX_ROWS) + 1) if upto[e] - upto[r] <= tile]
        out.append(max(ok) if ok else r + 1)
    return out


@pytest.mark.parametrize("seed", range(36))
def test_rowblocks_against_the_rule_stated_by_brute_force(seed):
    rng = np.random.default_rng(seed)
    tile = (64, 1024, 2048, 4096)[seed % 4]
    n = int(rng.integers(1, 3000))
    kind = seed % 3
    if kind == 0:          # mostly tiny rows (the 1024-row cap ends blocks), some of exactly tile / tile + 1 entries
        n += 1100
        lens = rng.integers(0, 2, size=n)
        for i in rng.integers(1024, n, size=4):      # (behind the first block: that one ends at the cap)
            lens[i] = tile + int(rng.integers(0, 2))
    elif kind == 1:        # the tile ends blocks
        lens = rng.integers(0, max(tile // 6, 2), size=n)
    else:                  # both, with runs of empty rows
        lens = rng.integers(0, 9, size=n) * (rng.random(n) < 0.3)
        lens[rng.integers(0, n)] = 3 * tile
    indptr = np.concatenate([[0], np.cumsum(lens)])
    got = cs.rowblocks(indptr, tile)
    assert list(got) == _brute_force_blocks(list(lens), tile)
    assert got[0] == 0 and got[-1] == n and np.all(np.diff(got) >= 1) and np.all(np.diff(got) <= cs.MAX_ROWS)
    if kind == 0 and tile >= 1024:
        assert got[1] == cs.MAX_ROWS
    if kind == 1 and got.size > 2:
        assert np.diff(got).max() < cs.MAX_ROWS and (np.diff(indptr[got]) > tile - tile // 6).any()


def _constant(text, name):
    m = re.search(r"constexpr\s+int\s+(?:[A-Z_]+\s*=\s*[^,;]+,\s*)*%s\s*=\s*([^,;]+)[,;]" % name, text)
    assert m, "constant %s not found" % name
    return m.group(1).strip()


def test_partial_slots_of_the_widest_grid_fit_the_allocation():
    """``k_cg_update`` writes one partial per workgroup from ``part_slot(SLOT_NRM)``, and ``grid_lin`` launches up to
    ``2 * nb <= 2 * NB_MAX`` workgroups; ``ctx->part`` holds ``(MAXC + 4) * NB_MAX`` doubles and slot ``s`` starts at
    ``s * NB_MAX``.  So ``2 * NB_MAX <= (MAXC + 4 - SLOT_NRM) * NB_MAX`` must hold - today with equality."""
    with open(os.path.join(CSRC, "kh_internal.h")) as f:
        internal = f.read()
    with open(os.path.join(CSRC, "krylov_steps.h")) as f:
        steps = f.read()
    with open(os.path.join(CSRC, "krylov_hip.hip")) as f:
        main = f.read()
    maxc = int(_constant(internal, "MAXC"))
    nb_max = int(_constant(internal, "NB_MAX"))
    slot_nrm = eval(_constant(steps, "SLOT_NRM"), {"__builtins__": {}}, {"MAXC": maxc})
    assert (maxc, nb_max, slot_nrm) == (16, 4096, 18)
    assert 2 * nb_max <= (maxc + 4 - slot_nrm) * nb_max
    # the three statements the inequality is built from, as the sources make them
    assert re.search(r"hipMalloc\(&ctx->part,\s*sizeof\(double\)\s*\*\s*\(size_t\)\(MAXC \+ 4\)\s*\*\s*NB_MAX\)", main)
    assert re.search(r"part_slot\(kh_ctx ctx, int slot\)\s*\{\s*return ctx->part \+ \(int64_t\)slot \* NB_MAX;", main)
    assert re.search(r"int grid_lin\(kh_ctx ctx, int64_t n\)\s*\{[^}]*std::min<int64_t>\(need, \(int64_t\)ctx->nb \* 2\)", main)
    assert re.search(r"KH_ARG\(reduce_blocks <= NB_MAX", main)
