"""Developer script (no GPU needed): is a move of kernels between source files a pure move?  Compiles two sets of .hip files to gfx950 device
assembly with build.sh's flags, cuts each .s into one piece per kernel and compares the pieces and the compiler's resource remarks.

    python tools/dev/isa_compare.py --old OLD_CSRC/kernels.hip --new iwae_amd/csrc/kernels.hip iwae_amd/csrc/wgrad_kernels.hip [--count-new iwae_amd/csrc/step_helpers.h] [--work DIR] [--flags=-DIWAE_DIAG]

A piece runs from the kernel's .globl line to its .Lfunc_end label; comments and the .file / .ident / __hip_cuid lines are dropped, and the
per-file function ordinal in local labels (.LBB<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n>) is rewritten away -- the ordinals number the
functions of a file and are the one thing a pure move changes.  Prints one line per kernel (identical / DIFFERS, VGPRs / AGPRs / scratch bytes per
lane / occupancy / LDS bytes of both sides), then the line counts; exit status 1 if a kernel was lost, added, doubled or differs."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -fno-slp-vectorize --cuda-device-only -S -Rpass-analysis=kernel-resource-usage"
FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "LDS"))


def compile_one(hipcc, src, work, tag, extra):
    out = os.path.join(work, "%s_%s" % (tag, os.path.basename(src)))
    cmd = [hipcc] + FLAGS.split() + extra + [os.path.basename(src), "-o", out + ".s"]
    r = subprocess.run(cmd, cwd=os.path.dirname(os.path.abspath(src)), stderr=subprocess.PIPE, text=True)
    with open(out + ".res", "w") as f:
        f.write(r.stderr)
    if r.returncode != 0:
        sys.exit("compile failed: %s\n%s" % (" ".join(cmd), r.stderr[-3000:]))
    return out


def pieces(path):
    """kernel symbol -> normalised assembly text; a symbol seen twice raises."""
    text = open(path + ".s").read().split("\n")
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(text), re.M))
    out, cur, name = {}, None, None
    for line in text:
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m and m.group(1) in kernels:
            name, cur = m.group(1), []
        if cur is None:
            continue
        if not (re.match(r"\s*(;|//)", line) or re.match(r"\s*\.(file|ident)\b", line) or "__hip_cuid" in line):
            line = re.sub(r"\s*;.*$", "", line)      # (trailing comments name blocks by ordinal too: "in Loop: Header=BB14_2")
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
            line = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", line)
            cur.append(line)
        if re.match(r"\.Lfunc_end:", line):
            if name in out:
                sys.exit("kernel defined twice in %s: %s" % (path, name))
            out[name], cur = "\n".join(cur), None
    return out


def resources(path):
    res, name = {}, None
    for line in open(path + ".res"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, short in FIELDS:
            m = re.search(r"remark:\s+%s: (\S+)" % re.escape(key), line)
            if m and name:
                res[name][short] = m.group(1)
    return res


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + list(names), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, text=True, check=True)
        return dict(zip(names, (re.sub(r"\(.*", "", l.replace("void ", "").replace("iwae::", "")) for l in r.stdout.split("\n"))))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--count-new", nargs="*", default=[], help="headers that came with the new files: counted with them in the line totals")
    ap.add_argument("--work", default="/tmp/isa_compare")
    ap.add_argument("--flags", default="", help="extra compiler flags, as --flags=-DIWAE_DIAG (a single flag given as a separate word is taken for an option)")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    jobs = [(f, "old") for f in a.old] + [(f, "new") for f in a.new]
    with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        outs = list(ex.map(lambda j: compile_one(a.hipcc, j[0], a.work, j[1], a.flags.split()), jobs))
    side = {"old": {}, "new": {}}
    where, resrc = {}, {"old": {}, "new": {}}
    bad = False
    for (src, tag), out in zip(jobs, outs):
        for k, v in pieces(out).items():
            if k in side[tag]:
                print("kernel in two files (%s): %s" % (tag, k))
                bad = True
            side[tag][k] = v
            if tag == "new":
                where[k] = os.path.basename(src)
        resrc[tag].update(resources(out))
    names = sorted(set(side["old"]) | set(side["new"]), key=lambda n: (where.get(n, ""), n))
    pretty = demangle(names)
    fmt = lambda r: " / ".join(r.get(s, "?") for _, s in FIELDS)
    print("# kernel | file | assembly | old: VGPRs / AGPRs / scratch / occupancy / LDS | new")
    ndiff = 0
    for n in names:
        if n not in side["old"] or n not in side["new"]:
            print("%-70s %s" % (pretty[n], "ADDED" if n not in side["old"] else "LOST"))
            bad = True
            continue
        same = side["old"][n] == side["new"][n]
        rsame = resrc["old"].get(n) == resrc["new"].get(n)
        ndiff += not (same and rsame)
        print("%-70s %-18s %-10s %-24s %-24s%s" % (pretty[n], where[n], "identical" if same else "DIFFERS", fmt(resrc["old"].get(n, {})), fmt(resrc["new"].get(n, {})),
                                                  "" if rsame else "   <-- resources differ"))
    print("# %d kernels in the old files, %d in the new; %d differ" % (len(side["old"]), len(side["new"]), ndiff))
    for tag, files in (("old", a.old), ("new", a.new + a.count_new)):
        cnt = [(os.path.basename(f), sum(1 for _ in open(f))) for f in files]
        print("# lines %s: %s = %d" % (tag, " + ".join("%s %d" % c for c in cnt), sum(c for _, c in cnt)))
    sys.exit(1 if bad or ndiff else 0)


if __name__ == "__main__":
    main()
