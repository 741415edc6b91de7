"""Developer script (GPU): A/B of a host-side change against a library built from its parent commit, through bench.py alone.

    python tools/dev/lib_ab.py dumps    --parent-lib PATH --out DIR  CASE ...
    python tools/dev/lib_ab.py launches --parent-lib PATH --out DIR  CASE ...
    python tools/dev/lib_ab.py timing   --parent-lib PATH --out DIR [--runs 8] CASE ...

CASE is "<config>:<precision>[:dist]", e.g. c1:fp32 or c1:bf16:dist (dist = bench.py --force-dist).
dumps:    bench.py --steps 30 --warmup 5 --dump-outputs on both builds; params, grads, adam_m, adam_v compared with numpy.array_equal.
launches: rocprofv3 --kernel-trace --stats (a run of its own, no counters) of bench.py --steps 30 --warmup 5 --settle 0 on both builds;
          per-kernel call counts side by side.
timing:   interleaved parent / this runs of bench.py --gpus 1 --steps 200 --warmup 20; this build's median against the parent's min..max.
Every child runs under its own time limit, and the script stops at the first child that does not exit with 0.  The text it prints (and
keeps in DIR/<mode>.txt) is what profiles/refactor_*_ab.txt and profiles/refactor_*_launches.txt are made of."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def child(cmd, limit, log):
    """Runs cmd under `timeout`; returns its stdout.  Any other exit status than 0 ends the script (nothing more is started on the GPU)."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    with open(log, "a") as f:
        f.write("$ %s\n[exit %d]\n%s\n%s\n" % (" ".join(cmd), r.returncode, r.stdout[-4000:], r.stderr[-4000:]))
    if r.returncode != 0:
        say("FAILED (exit %d): %s -- see %s" % (r.returncode, " ".join(cmd), log))
        finish(1)
    return r.stdout


def finish(rc):
    with open(os.path.join(ARGS.out, ARGS.mode + ".txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    sys.exit(rc)


def bench_cmd(case, lib, extra):
    parts = case.split(":")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", parts[0], "--precision", parts[1]] + extra
    if "dist" in parts[2:]:
        cmd.append("--force-dist")
    if lib:
        cmd += ["--lib", lib]
    return cmd


def result_line(stdout):
    return json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1])


def dumps():
    ok = True
    for case in ARGS.cases:
        ids = {}
        for who, lib in (("parent", ARGS.parent_lib), ("this", None)):
            d = os.path.join(ARGS.out, "dump_%s_%s" % (case.replace(":", "_"), who))
            out = child(bench_cmd(case, lib, ["--steps", "30", "--warmup", "5", "--dump-outputs", d]), 300, os.path.join(ARGS.out, "dumps.log"))
            ids[who] = result_line(out)["build_id"]
        import numpy as np
        eq = {}
        for name in ("params", "grads", "adam_m", "adam_v"):
            a, b = (np.load(os.path.join(ARGS.out, "dump_%s_%s" % (case.replace(":", "_"), who), name + ".npy")) for who in ("parent", "this"))
            eq[name] = bool(np.array_equal(a, b)) and a.size > 0
        ok = ok and all(eq.values())
        say("%-14s build_id parent %s this %s   %s" % (case, ids["parent"], ids["this"], "  ".join("%s %s" % (n, "equal" if e else "DIFFERS") for n, e in eq.items())))
    say("# every array equal (numpy.array_equal)" if ok else "# NOT all equal")
    finish(0 if ok else 1)


def launches():
    same = True
    for case in ARGS.cases:
        counts = {}
        for who, lib in (("parent", ARGS.parent_lib), ("this", None)):
            d = os.path.join(ARGS.out, "trace_%s_%s" % (case.replace(":", "_"), who))
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + bench_cmd(case, lib, ["--steps", "30", "--warmup", "5", "--settle", "0"])
            child(cmd, 400, os.path.join(ARGS.out, "launches.log"))
            rows = list(csv.DictReader(open(glob.glob(d + "/*/*kernel_stats.csv")[0])))
            counts[who] = {r["Name"]: int(r["Calls"]) for r in rows}
        say("## %s" % case.replace(":", " "))
        say("%-100s %8s %8s" % ("kernel", "parent", "this"))
        names = sorted(set(counts["parent"]) | set(counts["this"]), key=lambda n: (-counts["parent"].get(n, 0), n))
        for n in names:
            a, b = counts["parent"].get(n, 0), counts["this"].get(n, 0)
            same = same and a == b
            say("%-100s %8d %8d%s" % (n[:100], a, b, "" if a == b else "   <-- differs"))
        say("total launches: parent %d, this %d" % (sum(counts["parent"].values()), sum(counts["this"].values())))
        say()
    say("# every per-kernel call count is equal in all %d runs" % len(ARGS.cases) if same else "# call counts DIFFER")
    finish(0 if same else 1)


def timing():
    ms = {c: {"parent": [], "this": []} for c in ARGS.cases}
    ids = {}
    for run in range(ARGS.runs):
        for case in ARGS.cases:
            for who, lib in (("parent", ARGS.parent_lib), ("this", None)):
                r = result_line(child(bench_cmd(case, lib, ["--steps", "200", "--warmup", "20"]), 300, os.path.join(ARGS.out, "timing.log")))
                ms[case][who].append(r["ms_per_step"])
                ids[who] = r["build_id"]
                print("run %d %s %s %.4f" % (run + 1, case, who, r["ms_per_step"]), flush=True)
    say("# build_id: parent %s, this %s" % (ids["parent"], ids["this"]))
    cols = [(c, w) for c in ARGS.cases for w in ("parent", "this")]
    say("%-6s " % "run" + "".join("%-22s" % ("%s %s" % (c, w)) for c, w in cols))
    for run in range(ARGS.runs):
        say("%-6d " % (run + 1) + "".join("%-22.4f" % ms[c][w][run] for c, w in cols))
    say("%-6s " % "median" + "".join("%-22.5f" % statistics.median(ms[c][w]) for c, w in cols))
    inside = True
    for c in ARGS.cases:
        p, t = ms[c]["parent"], statistics.median(ms[c]["this"])
        ok = min(p) <= t <= max(p)
        inside = inside and (ok or t < min(p))
        say("# %s: parent spread (max - min) %.4f ms, %.4f .. %.4f; this build's median %.5f lies %s it (%+.2f us against the parent's median)."
            % (c, max(p) - min(p), min(p), max(p), t, "inside" if ok else "BELOW" if t < min(p) else "ABOVE", (t - statistics.median(p)) * 1000.0))
    finish(0 if inside else 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("dumps", "launches", "timing"))
    ap.add_argument("--parent-lib", required=True, help="libiwae_amd.so built from the parent commit")
    ap.add_argument("--out", required=True, help="directory for dumps, traces and logs")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("cases", nargs="+", metavar="CASE")
    ARGS = ap.parse_args()
    ARGS.parent_lib = os.path.abspath(ARGS.parent_lib)
    ARGS.out = os.path.abspath(ARGS.out)
    os.makedirs(ARGS.out, exist_ok=True)
    {"dumps": dumps, "launches": launches, "timing": timing}[ARGS.mode]()
