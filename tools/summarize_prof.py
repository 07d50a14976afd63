#!/usr/bin/env python
"""Summarise the rocprofv3 sqlite outputs of tools/profile.sh into a markdown file for profiles/.

  python tools/summarize_prof.py gpurun_out/prof_<tag> profiles/r01_<tag>.md

Kernel table = `rocprofv3 --kernel-trace --stats` (calls, total, average duration, share, VGPR /
SGPR / LDS).  HBM traffic = the FETCH_SIZE / WRITE_SIZE PMC passes, per launch, with the gfx950
correction of /opt/skills/guides/MI355X_MICROARCH.md (FETCH_SIZE reports 1/2 of the bytes of a
wide coalesced stream -> doubled; WRITE_SIZE is taken as reported, KiB).
"""
import json
import os
import sqlite3
import sys


def q(db, sql):
    con = sqlite3.connect(db)
    try:
        return con.execute(sql).fetchall()
    finally:
        con.close()


def short(name):
    name = name.replace("void kh::", "").replace("kh::", "")
    return name.split("(")[0]


def main(src, dst):
    lines = ["# rocprofv3 summary: %s" % os.path.basename(src.rstrip("/")), ""]
    bj = os.path.join(src, "bench_trace.json")
    if os.path.exists(bj):
        try:
            b = json.loads(open(bj).read().strip().splitlines()[-1])
            extra_args = " ".join(sys.argv[3:])
            lines += ["Command: `rocprofv3 --kernel-trace --stats -- python bench.py --full --steps %d --warmup %d "
                      "--no-cpu-baseline %s` (tools/profile.sh) on one MI355X; workload: %s" % (
                          b["steps"], b["warmup"], extra_args or ("--ortho %s --other-modes none" % b["config"].get("ortho")),
                          b["config"].get("workload", "")),
                      "", "bench.py under the profiler: **%.1f %s** (%.1f ms per step); "
                      "live HIP-event average of the dominant kernel `%s`: **%.3f us**." % (
                          b["value"], b["unit"], b["ms_per_step"], b["roofline"]["kernel"],
                          b["roofline"]["avg_launch_ms"] * 1e3), ""]
        except Exception as exc:  # pragma: no cover
            lines += ["(bench json unreadable: %r)" % exc, ""]
    tdb = os.path.join(src, "trace", "trace_results.db")
    rows = q(tdb, "select name,total_calls,total_duration,average,percentage from top_kernels")
    res = dict((r[0], r[1:]) for r in q(
        tdb, "select name, max(vgpr_count), max(sgpr_count), max(lds_size) from kernels group by name"))
    lines += ["## Kernel trace (`--kernel-trace --stats`)", "",
              "| kernel | calls | total ms | avg us | % | VGPR | SGPR | LDS B |", "|---|---:|---:|---:|---:|---:|---:|---:|"]
    for name, calls, tot, avg, pct in rows:
        v = res.get(name, ("", "", ""))
        lines.append("| `%s` | %d | %.2f | %.2f | %.2f | %s | %s | %s |" % (
            short(name), calls, tot / 1e3, avg, pct, v[0], v[1], v[2]))
    lines.append("")
    # bench.py's identical micro-launches (kh_bench_kernel) lie between two launches of `k_bench_marker` (an empty kernel the
    # harness issues in front of and behind its loop): selected by THAT - not by "the last N launches" (VERDICT r04:
    # kh_bench_arnoldi runs behind them since round 4) and not by a template argument (the orthogonality runs of bench.py
    # launch the same FND = 0 instantiation with other link counts)
    SOLVER_CHAIN = "name like '%k_mgs_chain%' and name not like '%, 0>%'"

    def between_markers(db, table, value, pat):
        marks = [r[0] for r in q(db, "select start from %s where name like '%%k_bench_marker%%' order by start" % table)]
        out = []
        for lo, hi in zip(marks[0::2], marks[1::2]):
            out += [r[0] for r in q(db, "select %s from %s where name like '%s' and start > %d and start < %d" % (value, table, pat, lo, hi))]
        return out

    try:
        d = between_markers(tdb, "kernels", "end - start", "%k_mgs_chain%")
        if d:
            lines.append("Kernel-trace average of the %d chain launches between the harness' markers (bench.py's 64-link "
                         "micro-launches, warm-up included): **%.1f us**." % (len(d), sum(d) / len(d) / 1e3))
        for pat, label in (("%k_cgs_dots%", "k_cgs_dots (16 columns)"), ("%k_cgs_update%", "k_cgs_update (16 columns)")):
            d = between_markers(tdb, "kernels", "end - start", pat)
            if d:
                lines.append("Kernel-trace average of the %d `%s` launches between the harness' markers (bench.py's "
                             "micro-launches): **%.1f us**." % (len(d), label, sum(d) / len(d) / 1e3))
        d = q(tdb, "select end - start from kernels where " + SOLVER_CHAIN)
        if d:
            lines.append("Kernel-trace average of all %d launches of the fused-operator chain kernel (the solver's Arnoldi "
                         "steps k >= 1; bench.py's `roofline.avg_launch_ms` averages the same launches plus step k = 0 and the "
                         "queue gaps): **%.1f us**." % (len(d), sum(x[0] for x in d) / len(d) / 1e3))
        lines.append("")
    except Exception as exc:  # pragma: no cover
        lines += ["(micro-launch durations unavailable: %r)" % exc, ""]
    def _pmc_between(db, cname, pat):
        marks = [r[0] for r in q(db, "select start from pmc_events where counter_name='%s' and name like '%%k_bench_marker%%' order by start" % cname)]
        out = []
        for lo, hi in zip(marks[0::2], marks[1::2]):
            out += [r[0] for r in q(db, "select counter_value from pmc_events where counter_name='%s' and name like '%s' and start > %d "
                                        "and start < %d" % (cname, pat, lo, hi))]
        return out

    pm = {}
    for cname in ("FETCH_SIZE", "WRITE_SIZE"):
        db = os.path.join(src, "pmc_" + cname, "pmc_results.db")
        if not os.path.exists(db):
            continue
        for name, n, avg in q(db, "select name, count(*), avg(counter_value) from pmc_events "
                                  "where counter_name='%s' group by name" % cname):
            pm.setdefault(name, {})[cname] = (n, avg)
    if pm:
        lines += ["## HBM traffic per launch (PMC passes, separate runs)", "",
                  "FETCH_SIZE / WRITE_SIZE are KiB per dispatch, averaged over all dispatches of the kernel. "
                  "`HBM read` = 2 x FETCH_SIZE (gfx950 correction for 16 B/lane coalesced streams), "
                  "`HBM write` = WRITE_SIZE.", "",
                  "| kernel | launches | FETCH_SIZE KiB | WRITE_SIZE KiB | HBM read MB | HBM write MB | total MB |",
                  "|---|---:|---:|---:|---:|---:|---:|"]
        for name, d in sorted(pm.items(), key=lambda kv: -kv[1].get("FETCH_SIZE", (0, 0))[0]):
            f = d.get("FETCH_SIZE", (0, 0.0))
            w = d.get("WRITE_SIZE", (0, 0.0))
            rd, wr = 2 * f[1] * 1024 / 1e6, w[1] * 1024 / 1e6
            lines.append("| `%s` | %d | %.0f | %.0f | %.1f | %.1f | %.1f |" % (
                short(name), f[0], f[1], w[1], rd, wr, rd + wr))
        lines.append("")
    # per-launch HBM traffic of the roofline kernel in bench.py's own micro-measurement: the last
    # launches of the run are kh_bench_kernel's identical 64-link (chain) launches
    tj = {}
    try:
        fdb = os.path.join(src, "pmc_FETCH_SIZE", "pmc_results.db")
        wdb = os.path.join(src, "pmc_WRITE_SIZE", "pmc_results.db")
        for key, pat, what in (("k_mgs_chain_micro", "%k_mgs_chain%", "chain launches"), ("k_cgs_dots", "%k_cgs_dots%", "k_cgs_dots launches"),
                               ("k_cgs_update", "%k_cgs_update%", "k_cgs_update launches")):
            f = [r for r in _pmc_between(fdb, "FETCH_SIZE", pat)]
            w = [r for r in _pmc_between(wdb, "WRITE_SIZE", pat)]
            if f and w:
                tj[key] = {"hbm_read_bytes_per_launch": 2 * sum(f) / len(f) * 1024, "hbm_write_bytes_per_launch": sum(w) / len(w) * 1024,
                           "launches_averaged": len(f),
                           "note": "the %d %s between the harness' k_bench_marker launches = bench.py's kh_bench_kernel launches; "
                                   "FETCH_SIZE doubled (gfx950 correction), separate --pmc passes" % (len(f), what)}
        # kernels of the secondary configurations' legs (bench.py --config 3 / 4 / 5): every launch of the run
        for key, pat in (("k_lanczos_fused", "%k_lanczos_fused%"), ("k_gemv_dense", "%k_gemv_dense%"), ("k_proj", "%k_proj_reg%")):
            f = q(fdb, "select counter_value from pmc_events where counter_name='FETCH_SIZE' and name like '%s'" % pat)
            w = q(wdb, "select counter_value from pmc_events where counter_name='WRITE_SIZE' and name like '%s'" % pat)
            if f and w:
                tj[key] = {"hbm_read_bytes_per_launch": 2 * sum(x[0] for x in f) / len(f) * 1024,
                           "hbm_write_bytes_per_launch": sum(x[0] for x in w) / len(w) * 1024, "launches_averaged": len(f),
                           "note": "all %d launches of the run; FETCH_SIZE doubled (gfx950 correction), separate --pmc passes" % len(f)}
        # per-dispatch durations of the stand-alone SpMV kernels (the plain instantiations, EPI = 0: bench.py's back-to-back
        # launches and nothing else) - what a kernel trace reproduces of the line's SpMV figures (the HIP-event
        # average of back-to-back launches sits below the per-dispatch average, whose every sample includes the kernel's own
        # ramp and drain)
        kt = {}
        for key, pat in (("k_spmv_dia", "%k_spmv_dia<0,%"), ("k_spmv_stream", "%k_spmv_stream<0,%")):
            d = q(tdb, "select end - start from kernels where name like '%s'" % pat)
            if d:
                kt[key] = {"avg_us": sum(x[0] for x in d) / len(d) / 1e3, "launches": len(d)}
        if kt:
            tj["kernel_trace_avg_us"] = kt
        # the solver's own instantiation of the chain kernel (operator in the prologue: a template argument FND > 0),
        # every launch of the run - whole cycles k = 1 .. m-1 of the solver and of kh_bench_arnoldi alike
        f = q(fdb, "select counter_value from pmc_events where counter_name='FETCH_SIZE' and " + SOLVER_CHAIN)
        w = q(wdb, "select counter_value from pmc_events where counter_name='WRITE_SIZE' and " + SOLVER_CHAIN)
        if f and w:
            rd = 2 * sum(x[0] for x in f) / len(f) * 1024
            wr = sum(x[0] for x in w) / len(w) * 1024
            tj["k_mgs_chain_solver"] = {
                "hbm_read_bytes_per_launch": rd, "hbm_write_bytes_per_launch": wr, "launches_averaged": len(f),
                "steps": "k >= 1",       # (step k = 0 runs the one-column Lanczos kernel: bench.py compares with the bytes of k >= 1)
                "note": "all %d launches of the fused-operator chain kernel in the run (Arnoldi steps k >= 1 of whole "
                        "GMRES cycles); FETCH_SIZE doubled (gfx950 correction), separate --pmc passes" % len(f)}
    except Exception as exc:  # pragma: no cover
        tj = {"error": repr(exc)}
    if tj and "error" not in tj:
        # tie the traffic numbers to the source tree they were measured on (bench.py attaches them to a
        # roofline line only when the stamp matches the kernels it has just timed)
        try:
            b = json.loads(open(bj).read().strip().splitlines()[-1])
            tj["source_stamp"] = b["roofline"]["source_stamp"]
            tj["n"] = int(b["config"]["n"])
        except Exception as exc:  # pragma: no cover
            tj["stamp_error"] = repr(exc)
    if tj:
        lines += ["## Roofline-kernel traffic (bench.py micro-launches)", "", "```json", json.dumps(tj, indent=1), "```", ""]
        with open(os.path.splitext(dst)[0] + "_traffic.json", "w") as fh:
            json.dump(tj, fh, indent=1)
    open(dst, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
