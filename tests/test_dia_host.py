"""CPU tests of the catalogue behind tests/test_gpu_dia.py (tests/support/dia_cases.py): every structure selects what it
claims under the restated upload plan, the plan itself agrees with truths written down by hand at the rule's boundaries, and
``edge_vector`` predicts exactly the rows whose product is not finite."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.support import dia_cases as dc


@pytest.mark.parametrize("name", dc.ALL)
def test_every_structure_selects_what_it_claims(name):
    c = dc.case(name)
    assert c.holds(), "%s: %s - plan %r" % (name, c.claim, c.plan())
    assert c.cplx == (name in dc.COMPLEX)
    assert c.n <= 18431
    mags = np.abs(np.concatenate([c.A.data.real, c.A.data.imag])) if c.cplx else np.abs(c.A.data)
    assert np.all((mags == 0) | ((mags >= 1) & (mags < 2))), "magnitudes in [1, 2)"


def test_the_catalogue_is_complete():
    for nd in dc.ND_COUNTS:
        assert "nd%d_value" % nd in dc.REAL and "nd%d_const" % nd in dc.REAL
    assert dc.ND_COUNTS == (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 32)
    for n in dc.ROW_EDGES:
        assert "edge%d_value" % n in dc.REAL and "edge%d_const" % n in dc.REAL
    # every template of k_spmv_dia in both forms where the form exists, and the generic loop in the mask form
    seen = set((dc.case(k).plan()["nd_template"], dc.case(k).plan()["masked"]) for k in dc.REAL if dc.case(k).plan()["banded"])
    assert seen == {(3, False), (5, False), (7, False), (9, False), (0, False), (3, True), (5, True), (7, True), (0, True)}
    assert sorted(dc.case(k).plan()["nd"] for k in dc.REAL if dc.case(k).plan()["masked"] and dc.case(k).plan()["nd_template"] == 0
                  and k.startswith("nd")) == [1, 2, 4, 6, 8]


def test_plan_against_hand_written_truths():
    def plan(name, rpt=4):
        return dc.dia_plan(dc.case(name).A, rpt)

    # the 70 % rule at n = 4100 with five diagonals: the bar is 14,350.0 exactly
    assert 0.7 * 5.0 * 4100.0 == 14350.0
    p = plan("threshold_in")
    assert dc.case("threshold_in").A.nnz == 14350
    assert (p["banded"], p["masked"], p["nd"], p["offsets"], p["nd_template"]) == (True, False, 5, (-2, -1, 0, 1, 2), 5)
    assert (p["rows_per_wg"], p["nblk"]) == (2048, 3)
    p = plan("threshold_out")
    assert dc.case("threshold_out").A.nnz == 14349
    assert (p["banded"], p["nd"], p["offsets"], p["nd_template"]) == (False, 5, (-2, -1, 0, 1, 2), 0)
    # the cap of 32 diagonals
    p = plan("nd32_value")
    assert (p["banded"], p["masked"], p["nd"], p["nd_template"], p["offsets"]) == (True, False, 32, 0, tuple(range(-16, 16)))
    p = plan("nd33")
    assert (p["banded"], p["nd"], p["offsets"]) == (False, 0, ())
    # n = 2
    p = plan("n2")
    assert (p["banded"], p["masked"], p["nd"], p["offsets"], p["nblk"]) == (True, False, 2, (0, 1), 1)
    p = plan("tri2")
    assert (p["banded"], p["nd"]) == (False, 3) and float(4) < 0.7 * 3.0 * 2.0
    one = sp.csr_matrix(np.array([[1.5]]))
    assert not dc.dia_plan(one)["banded"]                           # n = 1
    # n = 4 complex: 14 entries on a bar of exactly 14.0
    assert 0.7 * 5.0 * 4.0 == 14.0
    p = plan("z4")
    assert dc.case("z4").A.nnz == 14 and (p["banded"], p["masked"], p["nd"], p["nd_template"]) == (True, False, 5, 5)
    # constant but for one ulp; nine constant diagonals
    p = plan("one_ulp")
    assert (p["banded"], p["masked"], p["nd"], p["nd_template"]) == (True, False, 8, 0)
    p = plan("nd8_const")
    assert (p["banded"], p["masked"], p["nd"], p["nd_template"]) == (True, True, 8, 0)
    p = plan("nd9_const")
    assert (p["banded"], p["masked"], p["nd"], p["nd_template"]) == (True, False, 9, 9)
    A9 = dc.case("nd9_const").A
    off = A9.indices - np.repeat(np.arange(A9.shape[0]), np.diff(A9.indptr))
    assert all(np.unique(A9.data[off == o]).size == 1 for o in np.unique(off)), "nd9_const is constant on every diagonal"
    # complex: 5 or 7 only
    assert [plan(k)["banded"] for k in ("z3", "z5_513", "z7_513", "z9")] == [False, True, True, False]
    # geometry of the three measurement modes at the borders
    for n, want in ((2047, (4, 2, 1)), (2048, (4, 2, 1)), (2049, (5, 3, 2)), (16385, (33, 17, 9)), (18431, (36, 18, 9))):
        got = tuple(plan("edge%d_value" % n, rpt)["nblk"] for rpt in (1, 2, 4))
        assert got == want, (n, got)
        assert tuple(plan("edge%d_value" % n, rpt)["rows_per_wg"] for rpt in (1, 2, 4)) == (512, 1024, 2048)
    # a stored -0.0 is a stored zero; a purely imaginary entry is not
    A = dc.case("nd3_value").A.copy()
    A.data[5] = -0.0
    assert not dc.dia_plan(A)["banded"]
    A = dc.case("z5_513").A.copy()
    A.data[5] = 0.0
    assert not dc.dia_plan(A)["banded"]
    A.data[5] = 1.25j
    assert dc.dia_plan(A)["banded"]


def test_far7_is_what_the_issue_says():
    c = dc.case("far7_const")
    n = c.n
    assert n == 4099 and c.A.nnz == 20491 and 0.7 * 7.0 * 4099.0 > 20085.0 and 0.7 * 7.0 * 4099.0 < 20085.2
    x, rows = dc.edge_vector(c.A)
    assert list(rows) == [0, 1, 2, n - 3, n - 2, n - 1]
    assert x[0] == np.inf and x[n - 1] == -np.inf and np.isfinite(x[1:n - 1]).all()


@pytest.mark.parametrize("name", ["far7_value", "far7_const", "nd4_value", "nd4_const", "all_odd_value", "all_odd_const", "zfar7_4099",
                                  "z5_513", "z4", "edge3_const", "n2"])
def test_edge_vector_predicts_the_rows_that_are_not_finite(name):
    c = dc.case(name)
    x, rows = dc.edge_vector(c.A)
    with np.errstate(invalid="ignore", over="ignore"):
        y = c.A.dot(x)
    assert np.array_equal(np.flatnonzero(~np.isfinite(y)), rows), name
    assert 0 < rows.size < c.n or c.n <= 4


def test_vectors():
    x = dc.vector(1001, 3, seed=5)
    assert x.shape == (1001, 3) and x.flags.f_contiguous and np.all((np.abs(x) >= 1) & (np.abs(x) < 2))
    assert np.array_equal(x, dc.vector(1001, 3, seed=5)) and not np.array_equal(x, dc.vector(1001, 3, seed=6))
    z = dc.vector(11, 2, seed=5, cplx=True)
    assert z.dtype == np.complex128 and np.all((np.abs(z.real) >= 1) & (np.abs(z.imag) < 2))
