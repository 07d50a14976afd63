"""The chain-kernel dispatch, row by row (krypy_amd/csrc/chain_launch.hip): every case of tests/support/chain_dispatch_cases.py is
one upload and one Arnoldi / Lanczos step through kh_arnoldi_step_begin / _end (complex: kh_zarnoldi_step_begin_md) at the smallest
vector length that selects its row on 256 compute units.  Expected, from tests/golden/chain_dispatch.json - recorded by
tools/gen_chain_dispatch_golden.py BEFORE the launch layer was collected into one launcher and one dispatcher, twice, on an MI355X:
the same kernel family (the deltas of every launch counter) and the same bits (SHA-256 of the H column and of v_{k+1})."""
import json
import os

import pytest

from tests.support import chain_dispatch_cases as cd

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_dispatch.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_names_the_cases_of_the_table():
    assert sorted(GOLDEN["cases"]) == sorted(c["name"] for c in cd.CASES)


@pytest.mark.parametrize("c", cd.CASES, ids=[c["name"] for c in cd.CASES])
def test_same_kernel_and_same_bits_as_recorded(hip, c):
    assert hip.info()["compute_units"] == GOLDEN["compute_units"], "the sizes of the table select their rows on %d compute units" % GOLDEN["compute_units"]
    want = GOLDEN["cases"][c["name"]]
    got = cd.run_case(hip, c)
    print(c["name"], got)
    assert got["counters"] == want["counters"]
    if "h" in want:       # (cases whose bits were not stable run to run when recorded keep their counters only)
        assert (got["h"], got["v"]) == (want["h"], want["v"])
