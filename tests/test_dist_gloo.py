"""world_size-2 ... 8 CPU tests (gloo) of the block-row-sharded path: slab partition, column
localisation, halo exchange plan and all-reduced reductions, driven through the SAME host layer
(krypy_amd.dist.ShardedCSROperator + LinearSystem + RestartedGmres / DeflatedGmres / Minres).

RCCL itself cannot run here (no GPU); the NumPy test double routes the two exchanges through
torch.distributed/gloo instead, which proves the sharding logic the RCCL path relies on."""
import multiprocessing as mp
import os
import socket
import traceback

import numpy as np
import pytest

from oracle.inputs import lap2d_system, lap3d_system


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from krypy_amd import _hip
        from tests.support.numpy_context import GlooComm, NumpyContext

        ctx = NumpyContext(comm=GlooComm(rank, world))
        ctx.rank, ctx.nranks = rank, world
        _hip._install_context_for_testing(ctx)
        q.put((rank, "ok", case(rank, world, ctx)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "error", traceback.format_exc()))


def _run(case, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    for _ in range(world):
        rank, status, payload = q.get(timeout=600)
        assert status == "ok", payload
        out[rank] = payload
    for p in procs:
        p.join(timeout=60)
    return out


def _case_gmres(rank, world, ctx):
    from krypy_amd import dist as kdist, linsys, utils
    nx = 48
    A, b = lap2d_system(nx, rhs="rng1")
    cuts = kdist.slab_cuts(A.shape[0], world, align=nx)
    r0, r1 = cuts[rank], cuts[rank + 1]
    op = kdist.ShardedCSROperator(A[r0:r1], r0, A.shape[0], ctx)
    assert op.halo == ((nx if rank > 0 else 0), (nx if rank + 1 < world else 0),
                       (nx if rank > 0 else 0), (nx if rank + 1 < world else 0))
    if world == 5:
        assert [c // nx for c in cuts] == [0, 9, 19, 28, 38, 48]       # uneven slabs
    ls = linsys.LinearSystem(op, b[r0:r1])
    res = {}
    for ortho in ("mgs", "cgs2"):
        sol = linsys.RestartedGmres(ls, maxiter=40, max_restarts=30, tol=1e-8, ortho=ortho)
        res[ortho] = (np.array(sol.resnorms), sol.xk[:, 0].copy())
    return r0, r1, res


@pytest.mark.parametrize("world", [2, 5])
def test_sharded_restarted_gmres_matches_single_process(world):
    from oracle import krylov_ref as ref
    out = _run(_case_gmres, world)
    A, b = lap2d_system(48, rhs="rng1")
    o = ref.restarted_gmres(A, b, tol=1e-8, maxiter=40, max_restarts=30)
    for ortho in ("mgs", "cgs2"):
        x = np.zeros(A.shape[0])
        for rank, (r0, r1, res) in out.items():
            resn, xk = res[ortho]
            x[r0:r1] = xk
            assert len(resn) == len(o.resnorms)                     # same iteration count
            first = slice(0, 40)                                     # first cycle: 1e-10
            assert np.max(np.abs(resn[first] - np.array(o.resnorms)[first])
                          / np.array(o.resnorms)[first]) < 1e-10
        for r in range(1, world):
            assert np.array_equal(out[0][2][ortho][0], out[r][2][ortho][0])   # replicated scalars agree
        assert np.linalg.norm(A.dot(x) - b) <= 1.0001e-8 * np.linalg.norm(b)
        assert np.linalg.norm(x - o.xk) < 1e-7 * np.linalg.norm(o.xk)


def _case_deflated_and_minres(rank, world, ctx):
    from krypy_amd import deflation, dist as kdist, linsys
    nx = 12
    A, b = lap3d_system(nx, rhs="ones")
    N = A.shape[0]
    cuts = kdist.slab_cuts(N, world, align=nx * nx)
    r0, r1 = cuts[rank], cuts[rank + 1]
    op = kdist.ShardedCSROperator(A[r0:r1], r0, N, ctx)
    ls = linsys.LinearSystem(op, b[r0:r1], self_adjoint=True)
    U = np.random.default_rng(4).standard_normal((N, 5))
    s = deflation.DeflatedGmres(ls, U=U[r0:r1], tol=1e-9, maxiter=200, store_arnoldi=True)
    m = linsys.Minres(ls, tol=1e-9, maxiter=300)
    c = linsys.Cg(linsys.LinearSystem(op, b[r0:r1], self_adjoint=True, positive_definite=True),
                  tol=1e-9, maxiter=300)
    return r0, r1, np.array(s.resnorms), s.xk[:, 0].copy(), s.E, np.array(m.resnorms), \
        m.xk[:, 0].copy(), np.array(c.resnorms)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_deflated_gmres_minres_cg(world):
    """world 8: twelve planes of 144 rows over eight ranks - slabs of one and two planes (uneven), the one-plane
    slabs send their whole slab to both neighbours."""
    from oracle import krylov_ref as ref
    out = _run(_case_deflated_and_minres, world)
    A, b = lap3d_system(12, rhs="ones")
    U = np.random.default_rng(4).standard_normal((A.shape[0], 5))
    o = ref.deflated_gmres(A, b, U, tol=1e-9, maxiter=200)
    om = ref.minres(A, b, tol=1e-9, maxiter=300)
    oc = ref.cg(A, b, tol=1e-9, maxiter=300)
    x = np.zeros(A.shape[0])
    xm = np.zeros(A.shape[0])
    for rank, (r0, r1, resn, xk, E, mres, mx, cres) in out.items():
        x[r0:r1], xm[r0:r1] = xk, mx
        assert len(resn) == len(o.resnorms) and len(mres) == len(om.resnorms)
        assert len(cres) == len(oc.resnorms)
        assert np.max(np.abs(resn[:-1] - np.array(o.resnorms)[:-1]) / np.array(o.resnorms)[:-1]) < 1e-8
        assert np.linalg.norm(E - o.E) < 1e-10 * np.linalg.norm(o.E)
    assert np.linalg.norm(x - o.xk) < 1e-8 * np.linalg.norm(o.xk)
    assert np.linalg.norm(xm - om.xk) < 1e-7 * np.linalg.norm(om.xk)


def _case_complex(rank, world, ctx):
    from krypy_amd import deflation, dist as kdist, linsys
    from oracle.inputs import complex_systems
    c = complex_systems(24)
    A, b = c["nonh"], c["b"]
    N = A.shape[0]
    cuts = kdist.slab_cuts(N, world, align=24)
    r0, r1 = cuts[rank], cuts[rank + 1]
    op = kdist.ShardedCSROperator(A[r0:r1], r0, N, ctx)
    assert op.dtype.kind == "c" and op.halo[2] == (24 if rank > 0 else 0)
    ls = linsys.LinearSystem(op, b[r0:r1])
    s = linsys.Gmres(ls, tol=1e-10, maxiter=300)
    U = np.linalg.qr(np.random.default_rng(2).standard_normal((N, 4)) + 1j * np.random.default_rng(3).standard_normal((N, 4)))[0]
    sd = deflation.DeflatedGmres(ls, U=U[r0:r1], tol=1e-9, maxiter=300)
    # a REAL sharded matrix meeting a complex right-hand side: the c128 image of the slab and its halo
    opr = kdist.ShardedCSROperator(c["L"][r0:r1], r0, N, ctx)
    sr = linsys.Gmres(linsys.LinearSystem(opr, b[r0:r1]), tol=1e-10, maxiter=300)
    return r0, r1, np.array(s.resnorms), s.xk[:, 0].copy(), np.array(sd.resnorms), sd.xk[:, 0].copy(), \
        np.array(sr.resnorms), sr.xk[:, 0].copy()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_complex_gmres(world):
    """Complex (c128) block-row sharding: the halo carries (re, im) pairs, the inner products are all-reduced as
    pairs, the deflation projector runs inside the complex step - against the single-process complex oracle and the
    reference's golden run."""
    from oracle import krylov_ref_c as refc
    from oracle.inputs import complex_systems
    from tests.conftest import load_golden
    out = _run(_case_complex, world)
    c = complex_systems(24)
    A, b = c["nonh"], c["b"]
    g = load_golden("complex_nx24")
    xo, reso, _, _ = refc.gmres(A, b, tol=1e-10, maxiter=300)
    x = np.zeros(A.shape[0], dtype=complex)
    xd = np.zeros(A.shape[0], dtype=complex)
    xr = np.zeros(A.shape[0], dtype=complex)
    for rank, (r0, r1, resn, xk, dres, dx, rres, rx) in out.items():
        x[r0:r1], xd[r0:r1], xr[r0:r1] = xk, dx, rx
        assert len(resn) == len(reso) == len(g["gmres_resnorms"])
        assert np.max(np.abs(resn[:-1] - reso[:-1]) / reso[:-1]) < 1e-9
        assert len(rres) == len(g["gmres_realA_resnorms"])
    assert np.linalg.norm(x - xo) < 1e-8 * np.linalg.norm(xo)
    assert np.linalg.norm(x - g["gmres_xk"]) < 1e-8 * np.linalg.norm(xo)
    assert np.linalg.norm(A.dot(xd) - b) <= 1.01e-9 * np.linalg.norm(b)
    assert np.linalg.norm(xr - g["gmres_realA_xk"]) < 1e-8 * np.linalg.norm(xr)


def _case_complex_jacobi(rank, world, ctx):
    """Sharded complex CG / MINRES with a Jacobi preconditioner: the fused complex CG step (real recurrences on the
    real views, all-reduced <p, Ap> pair and <r, z>) and the complex step with its diagonal, on row slabs."""
    import scipy.sparse as sp
    from krypy_amd import dist as kdist, linsys
    from oracle.inputs import complex_systems
    nx = 24
    c = complex_systems(nx)
    b = c["b"]
    N = b.shape[0]
    cuts = kdist.slab_cuts(N, world, align=nx)
    r0, r1 = cuts[rank], cuts[rank + 1]
    d = np.asarray(c["hpd"].diagonal()).real[r0:r1]
    M, Minv = sp.diags(1.0 / d).tocsr(), sp.diags(d).tocsr()
    out = {}
    ctx.calls.clear()
    A = kdist.ShardedCSROperator(c["hpd"][r0:r1], r0, N, ctx)
    s = linsys.Cg(linsys.LinearSystem(A, b[r0:r1], M=M, Minv=Minv, self_adjoint=True, positive_definite=True),
                  tol=1e-10, maxiter=300)
    assert ctx.calls.get("cg_step") == len(s.resnorms) - 1, dict(ctx.calls)
    out["cg"] = (np.array(s.resnorms), s.xk[:, 0].copy())
    A = kdist.ShardedCSROperator(c["hind"][r0:r1], r0, N, ctx)
    ctx.calls.clear()
    s = linsys.Minres(linsys.LinearSystem(A, b[r0:r1], M=M, Minv=Minv, self_adjoint=True), tol=1e-10, maxiter=600)
    assert ctx.calls.get("dot_panel", 0) + ctx.calls.get("axpy_panel", 0) == 0, dict(ctx.calls)
    out["minres"] = (np.array(s.resnorms), s.xk[:, 0].copy())
    return r0, r1, out


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_complex_cg_minres_with_jacobi(world):
    import scipy.sparse as sp
    from oracle import krylov_ref_c as refc
    from oracle.inputs import complex_systems
    out = _run(_case_complex_jacobi, world)
    c = complex_systems(24)
    b = c["b"]
    M = sp.diags(1.0 / np.asarray(c["hpd"].diagonal()).real).tocsr()
    for name, A, fn, maxiter in (("cg", c["hpd"], refc.cg, 300), ("minres", c["hind"], refc.minres, 600)):
        xo, reso = fn(A, b, tol=1e-10, maxiter=maxiter, M=M)
        x = np.zeros(b.shape[0], dtype=complex)
        for rank, (r0, r1, res) in out.items():
            resn, xk = res[name]
            x[r0:r1] = xk
            assert len(resn) == len(reso), (name, len(resn), len(reso))
            assert np.max(np.abs(resn[:-1] - reso[:-1]) / reso[:-1]) < 1e-7, name
        assert np.linalg.norm(x - xo) < 1e-8 * np.linalg.norm(xo), name


def _bench_worker(rank, world, port, q):
    """bench.py exactly as `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` starts it (RANK /
    LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment), with the NumPy double standing in for the device."""
    try:
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        from krypy_amd import _hip
        from tests.support.numpy_context import NumpyContext
        ctx = NumpyContext()
        _hip._install_context_for_testing(ctx)
        import sys
        import bench
        sys.argv = ["bench.py", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--nx", "40", "--ny", "36",
                    "--restart", "12", "--no-roofline", "--no-cpu-baseline"]
        out, r, dist = bench._run()
        assert r == rank and ctx.nranks == world and ctx.rank == rank
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out))
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))


def _bench_self_spawn(argv, devices=8, timeout=600):
    """`python bench.py --gpus N ...` with NO launcher environment: bench.py starts its N ranks itself (bench._launch).
    tests/support/bench_double.py is bench.py with the NumPy double installed from the outside; the launcher re-executes
    that same command line for each rank."""
    import json
    import subprocess
    import sys
    env = dict((k, v) for k, v in os.environ.items()
               if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                            "KRYPY_AMD_DEVICE"))
    env["BENCH_DOUBLE_DEVICES"] = str(devices)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "support", "bench_double.py")] + argv, env=env,
                       cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    return p.returncode, lines, p.stderr.decode()


def _single_process_bench_residual(nx, ny, m, ortho="cgs"):
    from krypy_amd import _hip, linsys, utils
    from tests.support.numpy_context import NumpyContext
    import bench
    old = _hip._install_context_for_testing(NumpyContext())
    try:
        A = bench.laplace2d(nx, ny)
        b = np.random.default_rng(0).standard_normal(A.shape[0])
        ls = linsys.LinearSystem(A, b)
        x0 = None
        for ncyc in (1, 2):          # warm-up cycle, then the two timed ones from its iterate
            try:
                s = linsys.RestartedGmres(ls, x0=x0, maxiter=m, max_restarts=ncyc - 1, tol=1e-8, ortho=ortho)
            except utils.ConvergenceError as e:
                s = e.solver
            x0 = s.xk
        return s.resnorms[-1]
    finally:
        _hip._install_context_for_testing(old)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_bench_gpus_n_starts_its_own_ranks(world):
    """`python bench.py --gpus N` with a clean environment (what the driver runs for N = 1; what VERDICT r04 asked for
    N > 1): N rank processes are started by bench.py itself, exactly ONE JSON line comes back, it says n_gpus = N, and
    the iterations are the single-process ones."""
    import json
    rc, lines, err = _bench_self_spawn(["--gpus", str(world), "--steps", "2", "--warmup", "1", "--nx", "40", "--ny",
                                        "36", "--restart", "12", "--full", "--no-roofline", "--no-cpu-baseline"])
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    o = json.loads(lines[0])
    assert o["n_gpus"] == world and o["steps"] == 2 and o["warmup"] == 1 and o["unit"] == "iterations/s"
    # (--ortho auto: one untimed cycle of each candidate, the faster one is timed - either may win on the double)
    chosen = o["config"]["ortho"]
    assert chosen in ("cgs", "mgs") and o["config"]["iterations_timed"] == 24
    auto = o["config"]["ortho_auto"]
    assert auto["chosen"] == chosen and auto["chosen_transport"] == "rccl"
    assert [(c["ortho"], c["transport"]) for c in auto["candidates"]] == [("cgs", "rccl"), ("mgs", "rccl")]
    assert all("ms" in c for c in auto["candidates"]) and o["config"]["timed_region_fallback"] is None
    assert o["config"]["parallelism"] == "row-sharded x%d (RCCL)" % world
    assert o["value"] > 0 and abs(o["ms_per_step"] * 2 / 1e3 * o["value"] - 24) < 1e-6
    want = _single_process_bench_residual(40, 36, 12, ortho=chosen)
    assert abs(want - o["config"]["final_relres"]) <= 1e-9 * want
    assert o["config"]["basis_orthogonality_fro"][chosen] < 1e-10
    diag = o["config"]["sharded_diagnostics"]
    assert len(diag["rows_per_rank"]) == world and sum(diag["rows_per_rank"]) == 40 * 36 and len(diag["spmv_us_per_rank"]) == world


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py` line carries the headline and no extra measurement (those are `--full`'s); `--dump-outputs DIR`
    writes the timed run's iterate and residual history as float64, the same on one rank and on two."""
    import json
    argv = ["--steps", "2", "--warmup", "1", "--nx", "40", "--ny", "36", "--restart", "12", "--ortho", "cgs"]
    dumps = {}
    for world in (1, 2):
        d = str(tmp_path / ("w%d" % world))
        rc, lines, err = _bench_self_spawn(["--gpus", str(world), "--dump-outputs", d] + argv)
        assert rc == 0 and len(lines) == 1, err[-3000:]
        o = json.loads(lines[0])
        assert o["config"]["iterations_timed"] == 24 and abs(o["ms_per_step"] * 2 / 1e3 * o["value"] - 24) < 1e-6
        assert o["roofline"] is None and o["config"]["basis_orthogonality_fro"] is None
        assert o["config"]["sharded_diagnostics"] is None
        assert not {"cpu_baseline", "other_modes", "secondary"} & set(o)
        dumps[world] = dict((k, np.load(os.path.join(d, k + ".npy"))) for k in ("x", "resnorms"))
        assert all(a.dtype == np.float64 for a in dumps[world].values())
        assert dumps[world]["x"].shape == (40 * 36,) and dumps[world]["resnorms"].shape == (25,)
        assert dumps[world]["resnorms"][-1] == o["config"]["final_relres"]
    want = _single_process_bench_residual(40, 36, 12, ortho="cgs")
    assert abs(dumps[1]["resnorms"][-1] - want) <= 1e-9 * want
    assert np.linalg.norm(dumps[2]["x"] - dumps[1]["x"]) <= 1e-10 * np.linalg.norm(dumps[1]["x"])


def test_bench_gpus_n_refuses_when_fewer_devices_are_visible():
    """Never a silent N = 1: --gpus 4 with 2 visible devices exits non-zero, prints no JSON line and says why; so does
    a launcher environment that disagrees with --gpus (WORLD_SIZE = 1 included)."""
    import subprocess
    import sys
    rc, lines, err = _bench_self_spawn(["--gpus", "4", "--steps", "1", "--warmup", "0", "--nx", "40", "--ny", "36"],
                                       devices=2, timeout=120)
    assert rc != 0 and lines == [] and "only 2 GPUs visible" in err, (rc, lines, err[-500:])
    rc, lines, err = _bench_self_spawn(["--config", "5", "--gpus", "2", "--steps", "1", "--warmup", "0"], devices=1,
                                       timeout=120)
    assert rc != 0 and lines == [] and "only 1 GPU visible" in err, (rc, lines, err[-500:])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for cfg in ([], ["--config", "5"]):
        env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "support", "bench_double.py"), "--gpus", "2",
                            "--steps", "1", "--warmup", "0"] + cfg, env=env, cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=120)
        assert p.returncode != 0 and p.stdout.strip() == b"" and b"WORLD_SIZE=1" in p.stderr, p.stderr[-500:]


def test_bench_loop_halo_needs_the_forced_one_rank_path():
    """`--loop-halo` (one rank as a middle slab, its own neighbour) means something on ONE rank in forced multi-rank mode only:
    anywhere else the command line is refused - it is not silently a different measurement."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for argv in (["--loop-halo"], ["--loop-halo", "--force-sharded", "--gpus", "2"]):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + argv + ["--steps", "1", "--warmup", "0"], cwd=root,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode != 0 and p.stdout.strip() == b"" and b"--loop-halo" in p.stderr, p.stderr[-500:]


def test_bench_gpus_n_reports_a_failed_rank():
    """A rank that dies must not leave the launcher waiting nor a JSON line behind: here every rank fails at argument
    checks that only the rank processes run (restart length larger than the local slab allows is fine; an unknown
    Gram-Schmidt variant is not)."""
    rc, lines, err = _bench_self_spawn(["--gpus", "2", "--steps", "1", "--warmup", "0", "--nx", "40", "--ny", "36",
                                        "--restart", "12", "--ortho", "no-such-variant", "--no-roofline",
                                        "--no-cpu-baseline"], timeout=300)
    assert rc != 0 and lines == [] and "ranks failed" in err, (rc, lines, err[-800:])


def test_bench_ortho_auto_goes_back_to_the_panel_form_when_the_candidate_fails():
    """`--ortho auto` on N > 1 ranks times one untimed cycle of `cgs` and of `mgs` and takes the faster - and the `mgs` candidate is
    the one whose in-launch sums have never crossed a link between two GPUs.  When it fails (here: every rank's reference-order step
    raises at k = 5, what a timed-out sum looks like from the host) the run must not lose its line: every rank goes back to the
    panel form together, the line says so, and the timed cycles are the `cgs` ones of an undisturbed run."""
    import json
    os.environ["BENCH_DOUBLE_FAIL_MGS_AT"] = "5"
    try:
        rc, lines, err = _bench_self_spawn(["--gpus", "2", "--steps", "2", "--warmup", "1", "--nx", "40", "--ny", "36",
                                            "--restart", "12", "--no-roofline", "--no-cpu-baseline"])
    finally:
        del os.environ["BENCH_DOUBLE_FAIL_MGS_AT"]
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    o = json.loads(lines[0])
    assert o["n_gpus"] == 2 and o["config"]["ortho"] == "cgs" and o["config"]["iterations_timed"] == 24
    auto = o["config"]["ortho_auto"]
    assert auto["chosen"] == "cgs" and "ms_per_cycle" in auto["cgs"]
    assert "told to fail at k = 5" in auto["mgs"]["error"] and "panel form" in auto["mgs"]["disabled"]
    assert "ms_per_cycle" not in auto["mgs"]
    want = _single_process_bench_residual(40, 36, 12)
    assert abs(want - o["config"]["final_relres"]) <= 1e-9 * want


def test_bench_timed_region_falls_back_to_the_panel_form_together():
    """A failure INSIDE the timed region (what a sum over the mailboxes that times out looks like from the host -
    an error on every rank of the communicator, here from the 20th reference-order step on, i.e. in the second cycle of the region)
    must not cost the run its line where there is something to go back to: every rank reports through the same host collective, all
    of them switch to the panel form over RCCL, the region is timed again, and the line says so.  Bounded: well under a minute."""
    import json
    import time
    os.environ["BENCH_DOUBLE_FAIL_MGS_AFTER"] = "20"
    try:
        t0 = time.time()
        rc, lines, err = _bench_self_spawn(["--gpus", "2", "--steps", "2", "--warmup", "1", "--nx", "40", "--ny", "36", "--restart", "12",
                                            "--ortho", "mgs", "--no-roofline", "--no-cpu-baseline", "--other-modes", "none"])
        took = time.time() - t0
    finally:
        del os.environ["BENCH_DOUBLE_FAIL_MGS_AFTER"]
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    o = json.loads(lines[0])
    fb = o["config"]["timed_region_fallback"]
    assert fb is not None and fb["from"] == {"ortho": "mgs", "transport": "rccl"} and "told to fail" in fb["reason"]
    assert o["config"]["ortho"] == "cgs" and o["config"]["iterations_timed"] == 24 and o["n_gpus"] == 2
    want = _single_process_bench_residual(40, 36, 12, ortho="cgs")
    assert abs(want - o["config"]["final_relres"]) <= 1e-9 * want
    assert took < 120.0, took


def test_bench_gpus_n_stops_the_others_when_one_rank_dies():
    """ONE rank dies before the rendezvous while rank 0 waits there for it: the launcher must see the dead rank although rank 0
    has not closed its stdout, stop the waiting ranks (its own children, by PID) and report - not sit in a read of rank 0's
    pipe until the rendezvous' own ten-minute timeout."""
    import time
    os.environ["BENCH_DOUBLE_DIE_RANK"] = "1"
    try:
        t0 = time.time()
        rc, lines, err = _bench_self_spawn(["--gpus", "2", "--steps", "1", "--warmup", "0", "--nx", "40", "--ny", "36",
                                            "--restart", "12", "--no-roofline", "--no-cpu-baseline"], timeout=200)
        took = time.time() - t0
    finally:
        del os.environ["BENCH_DOUBLE_DIE_RANK"]
    assert rc != 0 and lines == [] and "ranks failed" in err and "(1, 3)" in err, (rc, lines, err[-800:])
    assert took < 120.0, took


def test_bench_sharded_path_under_an_external_launcher():
    """The same leg as a launcher (`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`) starts it:
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment.  Every rank reports the same (max-over-ranks) time and
    the same residual."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bench_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = {}
    for _ in range(world):
        rank, status, payload = q.get(timeout=600)
        assert status == "ok", payload
        outs[rank] = payload
    for p in procs:
        p.join(timeout=60)
    o = outs[0]
    assert o["n_gpus"] == world and o["config"]["iterations_timed"] == 24
    assert len({round(outs[r]["value"], 6) for r in outs}) == 1
    assert len({outs[r]["config"]["final_relres"] for r in outs}) == 1
    assert len({outs[r]["config"]["ortho"] for r in outs}) == 1            # every rank timed the same candidate
    want = _single_process_bench_residual(40, 36, 12, ortho=o["config"]["ortho"])
    assert abs(want - o["config"]["final_relres"]) <= 1e-9 * want


def _bench5_worker(rank, world, port, q):
    """bench.py --config 5 as torch.distributed.run starts it, NumPy double as the device."""
    try:
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        from krypy_amd import _hip
        from tests.support.numpy_context import NumpyContext
        ctx = NumpyContext()
        _hip._install_context_for_testing(ctx)
        import sys
        import bench
        sys.argv = ["bench.py", "--config", "5", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--nx", "12",
                    "--ny", "10", "--nz", "16", "--restart", "30", "--defl", "5", "--no-cpu-baseline"]
        out, r, dist = bench._run()
        assert r == rank and ctx.nranks == world and ctx.rank == rank
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out))
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 4, 8])
def test_bench_config5_leg_on_n_ranks(world):
    """The config-5 leg of bench.py (z-slabs of the 3-D grid, plain GMRES to harvest Ritz vectors that stay sharded on
    the device, DeflatedGmres timed) on gloo ranks at a toy size: same JSON contract as config 2, every rank sees the
    same numbers, and those are the CPU oracle's (gmres -> Ritz vectors of smallest magnitude -> deflated_gmres;
    reference flow recycling/linsys.py:51-103, deflation.py:93-163).  world = 2: under an external launcher's
    environment (all ranks' lines compared); world = 4 and 8 (BASELINE.json configs[4]'s partition: two-plane slabs here):
    `bench.py --config 5 --gpus N` starting its own ranks."""
    if world >= 4:
        import json
        rc, lines, err = _bench_self_spawn(["--config", "5", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--nx", "12",
                                            "--ny", "10", "--nz", "16", "--restart", "30", "--defl", "5",
                                            "--no-cpu-baseline"])
        assert rc == 0 and len(lines) == 1, err[-3000:]
        outs = {0: json.loads(lines[0])}
    else:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_bench5_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        outs = {}
        for _ in range(world):
            rank, status, payload = q.get(timeout=600)
            assert status == "ok", payload
            outs[rank] = payload
        for p in procs:
            p.join(timeout=60)
    o = outs[0]
    assert o["n_gpus"] == world and o["steps"] == 2 and o["unit"] == "iterations/s" and o["scaling"] == "strong"
    assert o["config"]["iterations_timed"] == 60 and o["config"]["deflation_vectors"] == 5
    assert o["config"]["parallelism"] == "z-slabs x%d (RCCL)" % world and o["config"]["ortho"] in ("cgs", "mgs")
    assert o["config"]["ortho_auto"]["chosen"]["ortho"] == o["config"]["ortho"] and o["config"]["timed_region_fallback"] is None
    assert o["value"] > 0 and abs(o["ms_per_step"] * 2 / 1e3 * o["value"] - 60) < 1e-6
    for key in ("plain_relres", "deflated_relres"):
        assert len({outs[r]["config"][key] for r in outs}) == 1, key
    import bench
    from oracle import krylov_ref as ref
    A = bench.laplace3d(12, 10, 16)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    o0 = ref.gmres(A, b, tol=1e-12, maxiter=30)
    vals, U = ref.ritz_vectors_smallest(o0, 5, self_adjoint=True)
    o1 = ref.deflated_gmres(A, b, U, tol=1e-12, maxiter=30)
    assert abs(o["config"]["plain_relres"] - o0.resnorms[-1]) <= 1e-8 * o0.resnorms[-1]
    assert np.allclose(o["config"]["smallest_ritz_values"], np.sort(np.abs(vals))[:4], rtol=1e-8)
    assert abs(o["config"]["deflated_relres"] - o1.resnorms[-1]) <= 1e-6 * o1.resnorms[-1]
    assert o["config"]["deflated_relres"] < o["config"]["plain_relres"]


def test_slab_cuts_and_localize():
    from krypy_amd import dist as kdist
    assert kdist.slab_cuts(100, 4) == [0, 25, 50, 75, 100]
    assert kdist.slab_cuts(2500 * 4000, 8, align=4000)[1] == 312 * 4000
    cuts = kdist.slab_cuts(10, 3, align=4)
    assert cuts[0] == 0 and cuts[-1] == 10 and all(a <= b for a, b in zip(cuts, cuts[1:]))
    A, _ = lap2d_system(6, rhs="ones")
    Al, nrp, nrn = kdist.localize_columns(A[12:24], 12, 36)
    assert (nrp, nrn) == (6, 6) and Al.shape == (12, 24)
    x = np.arange(36.0)
    xl = np.concatenate([x[12:24], x[6:12], x[24:30]])
    assert np.array_equal(Al.dot(xl), A[12:24].dot(x))
    Al, nrp, nrn = kdist.localize_columns(A[0:12], 0, 36)
    assert (nrp, nrn) == (0, 6)


def _rdv_worker(rank, world, port, q):
    try:
        from krypy_amd.dist import TcpRendezvous
        r = TcpRendezvous(rank, world, addr="127.0.0.1", port=port, timeout=120.0)
        uid = r.broadcast_bytes(bytes(range(128)) if rank == 0 else None)
        r.barrier()
        m = r.allreduce_max(10.0 + rank)
        m2 = r.allreduce_max(-float(rank))
        r.barrier()
        r.close()
        q.put((rank, "ok", (uid, m, m2)))
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))


@pytest.mark.parametrize("world", [1, 2, 5])
def test_tcp_rendezvous_broadcast_barrier_max(world):
    """krypy_amd.dist.TcpRendezvous is all the launcher-side plumbing bench.py needs for N > 1 (the ncclUniqueId to
    every rank, a barrier, the max over ranks of the elapsed time) - plain sockets, no torch.distributed."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rdv_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = {}
    for _ in range(world):
        rank, status, payload = q.get(timeout=300)
        assert status == "ok", payload
        outs[rank] = payload
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        uid, m, m2 = outs[r]
        assert uid == bytes(range(128)) and m == 10.0 + world - 1 and m2 == 0.0
