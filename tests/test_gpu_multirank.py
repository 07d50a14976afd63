"""`bench.py --gpus N` on real devices (VERDICT r04 "missing 1").

Rounds 1-4 never put two ranks through RCCL: every box had one GPU.  These tests adapt to the box:
* one visible GPU (today's boxes): `--gpus 2` must REFUSE - non-zero exit, a reason on stderr, no JSON line - for config 2
  and config 5 alike (never a silent n_gpus = 1 run);
* two or more visible GPUs: `python bench.py --gpus 2` with a clean environment starts two rank processes by itself
  (one per device, RCCL communicator, halo exchange + all-reduced dots), prints ONE line with n_gpus = 2, and the
  iterations are the one-GPU ones (the sharded operator replaces /root/reference/krypy/utils.py:1593-1594, the
  all-reduced inner products utils.py:182-183).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LAUNCHER_VARS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                  "KRYPY_AMD_DEVICE", "KRYPY_AMD_FORCE_MULTI")


def _bench(argv, timeout=900):
    env = dict((k, v) for k, v in os.environ.items() if k not in _LAUNCHER_VARS)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    return p.returncode, lines, p.stderr.decode()


def test_bench_gpus_n_refuses_without_n_devices(hip):
    from krypy_amd import _hip
    have = _hip.device_count()
    assert have >= 1
    want = have + 1
    for cfg in ([], ["--config", "5"]):
        rc, lines, err = _bench(["--gpus", str(want), "--steps", "1", "--warmup", "0", "--nx", "64", "--ny", "48"] + cfg,
                                timeout=300)
        assert rc != 0 and lines == [], (rc, lines)
        assert "only %d GPU" % have in err, err[-600:]


def test_bench_two_real_ranks_match_one(hip):
    from krypy_amd import _hip
    if _hip.device_count() < 2:
        pytest.skip("one GPU on this box: the two-rank RCCL run needs two (the refusal test above ran instead)")
    common = ["--steps", "2", "--warmup", "1", "--nx", "400", "--ny", "300", "--restart", "40", "--no-cpu-baseline",
              "--no-roofline", "--ortho", "cgs", "--other-modes", "none"]
    rc, lines, err = _bench(["--gpus", "2"] + common)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    two = json.loads(lines[0])
    assert two["n_gpus"] == 2 and two["config"]["parallelism"] == "row-sharded x2 (RCCL)"
    assert two["config"]["iterations_timed"] == 80
    rc, lines, err = _bench(["--gpus", "1"] + common)
    assert rc == 0 and len(lines) == 1, err[-3000:]
    one = json.loads(lines[0])
    assert one["n_gpus"] == 1
    r1, r2 = one["config"]["final_relres"], two["config"]["final_relres"]
    assert abs(r1 - r2) <= 1e-9 * r1, (r1, r2)
    # reference-order MGS on two ranks (one all-reduce of 2k + 1 values per step) against the same
    rc, lines, err = _bench(["--gpus", "2"] + [a if a != "cgs" else "mgs" for a in common])
    assert rc == 0 and len(lines) == 1, err[-3000:]
    two_mgs = json.loads(lines[0])
    rc, lines, err = _bench(["--gpus", "1"] + [a if a != "cgs" else "mgs" for a in common])
    one_mgs = json.loads(lines[0])
    r1, r2 = one_mgs["config"]["final_relres"], two_mgs["config"]["final_relres"]
    assert abs(r1 - r2) <= 1e-9 * r1, (r1, r2)


def test_bench_two_ranks_share_the_one_gpu_through_the_mailboxes(hip):
    """The whole N > 1 path of bench.py on a box with ONE GPU: `python bench.py --gpus 2 --share-devices --transport xr` starts
    two rank processes by itself, both on device 0, with NO RCCL communicator (RCCL refuses two ranks on one device): the sums
    across the ranks through the IPC mailboxes (csrc/xr.hip), the halo of the two slabs inside the banded SpMV's own launch
    (xh), the reference-order candidate of `--ortho auto` through the blocked kernel with the exchange inside its launch
    (chain_blk2.h).  ONE line comes back; it says two ranks on one device, which transports ran, and the residual after the
    same iterations is the one-rank run's (the sharded operator: /root/reference/krypy/utils.py:1593-1594, the summed inner
    products: utils.py:182-183)."""
    common = ["--steps", "2", "--warmup", "1", "--nx", "400", "--ny", "300", "--restart", "40", "--no-cpu-baseline",
              "--no-roofline", "--other-modes", "none"]
    res = {}
    for ortho in ("cgs", "mgs", "auto"):
        rc, lines, err = _bench(["--gpus", "2", "--share-devices", "--transport", "xr", "--ortho", ortho] + common)
        assert rc == 0, err[-3000:]
        assert len(lines) == 1, lines
        two = json.loads(lines[0])
        c = two["config"]
        assert two["n_gpus"] == 1 and c["ranks"] == 2 and c["parallelism"] == "row-sharded x2 (mailboxes only)"
        assert c["cross_rank_sums"] == "xr" and c["halo"] == "in-launch" and c["iterations_timed"] == 80
        res[ortho] = two
    assert res["auto"]["config"]["ortho"] in ("cgs", "mgs") and set(res["auto"]["config"]["ortho_auto"]) >= {"cgs", "mgs", "chosen"}
    cands = res["auto"]["config"]["ortho_auto"]["candidates"]
    assert [(c_["ortho"], c_["transport"]) for c_ in cands] == [("cgs", "xr"), ("mgs", "xr")] and all("ms" in c_ for c_ in cands)
    assert cands[1]["kernels"]["blocked_in_launch_sums"] > 0 and cands[1]["per_iteration"]["allreduce_calls"] < 1.0
    for ortho in ("cgs", "mgs"):
        rc, lines, err = _bench(["--gpus", "1", "--ortho", ortho] + common)
        assert rc == 0 and len(lines) == 1, err[-3000:]
        one = json.loads(lines[0])
        r1, r2 = one["config"]["final_relres"], res[ortho]["config"]["final_relres"]
        assert abs(r1 - r2) <= 1e-9 * r1, (ortho, r1, r2)


def test_bench_one_rank_as_a_middle_slab_with_itself_as_neighbour(hip):
    """`bench.py --force-sharded --loop-halo`: what ONE middle rank of N runs, kernel for kernel, on a box with one GPU - the
    sums through its own mailbox inside the blocked kernel's launch, its boundary rows out and its ghost rows in inside the
    banded SpMV's launch (the slab periodic across its cuts).  The line says so, and the residual after the same iterations
    is the one the RCCL exchange (two launches and a send / recv kernel per product, KRYPY_AMD_XH=0) arrives at."""
    common = ["--force-sharded", "--loop-halo", "--steps", "2", "--warmup", "1", "--nx", "400", "--ny", "300", "--restart", "40",
              "--no-cpu-baseline", "--no-roofline", "--ortho", "mgs", "--other-modes", "none"]
    rc, lines, err = _bench(common)
    assert rc == 0 and len(lines) == 1, err[-3000:]
    a = json.loads(lines[0])
    assert a["config"]["halo"] == "in-launch (the slab is its own neighbour)" and a["config"]["cross_rank_sums"] == "xr"
    os.environ["KRYPY_AMD_XH"] = "0"
    try:
        rc, lines, err = _bench(common)
    finally:
        del os.environ["KRYPY_AMD_XH"]
    assert rc == 0 and len(lines) == 1, err[-3000:]
    b = json.loads(lines[0])
    assert b["config"]["halo"] == "rccl (the slab is its own neighbour)"
    r1, r2 = a["config"]["final_relres"], b["config"]["final_relres"]
    assert abs(r1 - r2) <= 1e-9 * r1, (r1, r2)


def test_bench_timed_region_fallback_on_the_real_context(hip):
    """A failure INSIDE the timed region of a sharded run (here faked: the first launch with in-launch sums of the region
    reports a timed-out sum, `KRYPY_AMD_BENCH_FAULT=1`; on a communicator that is KH_ERR_COMM, never a rank-local recovery)
    must not cost the run its line: the mailboxes are detached, the halo goes back to ncclSend / ncclRecv, the panel form over
    ncclAllReduce is timed instead - on the REAL context (the CPU suite runs the same logic on the double) - and the line says
    so; the residual is the one of a plain `--ortho cgs` run over RCCL."""
    common = ["--force-sharded", "--steps", "2", "--warmup", "1", "--nx", "4000", "--ny", "700", "--restart", "30", "--full",
              "--no-cpu-baseline", "--no-roofline", "--other-modes", "none"]
    os.environ["KRYPY_AMD_BENCH_FAULT"] = "1"
    try:
        rc, lines, err = _bench(common + ["--ortho", "mgs"])
    finally:
        del os.environ["KRYPY_AMD_BENCH_FAULT"]
    assert rc == 0 and len(lines) == 1, err[-3000:]
    a = json.loads(lines[0])
    fb = a["config"]["timed_region_fallback"]
    assert fb is not None and fb["from"] == {"ortho": "mgs", "transport": "xr"} and "timed out" in fb["reason"], fb
    assert a["config"]["ortho"] == "cgs" and a["config"]["cross_rank_sums"] == "rccl" and a["config"]["halo"].startswith("rccl")
    assert a["config"]["iterations_timed"] == 60 and a["config"]["sharded_diagnostics"]["per_iteration"]["n_xr"] == 0
    os.environ["KRYPY_AMD_XR"] = "0"
    try:
        rc, lines, err = _bench(common + ["--ortho", "cgs"])
    finally:
        del os.environ["KRYPY_AMD_XR"]
    assert rc == 0 and len(lines) == 1, err[-3000:]
    b = json.loads(lines[0])
    r1, r2 = a["config"]["final_relres"], b["config"]["final_relres"]
    assert abs(r1 - r2) <= 1e-9 * r1, (r1, r2)


def test_bench_config5_two_ranks_share_the_one_gpu(hip):
    """BASELINE.json configs[4]'s flow (harvest of the Ritz vectors on the device, DeflatedGmres with them:
    /root/reference/krypy/recycling/linsys.py:51-103, deflation.py:93-163) on TWO rank processes, z-slabs of the 3-D
    Laplacian, on a box with one GPU: no RCCL communicator - every inner product, the projector's panel products and the
    host-side sums through the mailboxes, the slabs' halo planes inside the banded SpMV's launch.  The deflated residual
    after the same iterations is the one-rank run's (Ritz values too): the first time this flow runs on more than one rank."""
    common = ["--config", "5", "--steps", "1", "--warmup", "0", "--nx", "40", "--ny", "36", "--nz", "30", "--restart", "30",
              "--defl", "6", "--no-cpu-baseline", "--no-roofline"]
    res = {}
    for ortho in ("cgs", "mgs"):
        rc, lines, err = _bench(["--gpus", "2", "--share-devices", "--transport", "xr", "--ortho", ortho] + common)
        assert rc == 0, err[-3000:]
        assert len(lines) == 1, lines
        two = json.loads(lines[0])
        c = two["config"]
        assert two["n_gpus"] == 1 and c["ranks"] == 2 and c["parallelism"] == "z-slabs x2 (mailboxes only)"
        assert c["cross_rank_sums"] == "xr" and c["halo"] == "in-launch" and c["iterations_timed"] == 30
        res[ortho] = two
        rc, lines, err = _bench(["--gpus", "1", "--ortho", ortho] + common)
        assert rc == 0 and len(lines) == 1, err[-3000:]
        one = json.loads(lines[0])["config"]
        assert abs(one["plain_relres"] - c["plain_relres"]) <= 1e-8 * one["plain_relres"], (ortho, one["plain_relres"], c["plain_relres"])
        assert abs(one["deflated_relres"] - c["deflated_relres"]) <= 1e-6 * one["deflated_relres"], (ortho, one["deflated_relres"], c["deflated_relres"])
        assert np.allclose(one["smallest_ritz_values"], c["smallest_ritz_values"], rtol=1e-8)


@pytest.mark.parametrize("ranks", [3, 4])
def test_bench_middle_ranks_share_the_one_gpu(hip, ranks):
    """Three and four rank processes on the one device (`--share-devices --transport xr`): ranks with TWO neighbours - both
    ghost regions of a slab filled from two other processes inside the SpMV's launch, a sum across more than two mailboxes, an
    uneven split of the rows (300 = 75 x 4, 100 x 3; the Gram-Schmidt kernels are chosen for the longest slab) - against one
    rank: the same residual after the same iterations, panel form and reference order."""
    common = ["--steps", "2", "--warmup", "1", "--nx", "400", "--ny", "300", "--restart", "40", "--no-cpu-baseline",
              "--no-roofline", "--other-modes", "none"]
    for ortho in ("cgs", "mgs"):
        rc, lines, err = _bench(["--gpus", str(ranks), "--share-devices", "--transport", "xr", "--ortho", ortho] + common)
        assert rc == 0 and len(lines) == 1, err[-3000:]
        many = json.loads(lines[0])
        c = many["config"]
        assert many["n_gpus"] == 1 and c["ranks"] == ranks and c["cross_rank_sums"] == "xr" and c["halo"] == "in-launch"
        rc, lines, err = _bench(["--gpus", "1", "--ortho", ortho] + common)
        assert rc == 0 and len(lines) == 1, err[-3000:]
        one = json.loads(lines[0])["config"]
        assert abs(one["final_relres"] - c["final_relres"]) <= 1e-9 * one["final_relres"], (ortho, one["final_relres"], c["final_relres"])
