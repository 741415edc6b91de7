"""Developer script (no GPU needed): instruction mix per basic block of one kernel in the gfx950 ISA of the step's kernel files.
usage: python tools/dev/isa_mix.py <mangled-name-substring> [min MFMAs per block to print] [file.hip ...]
(compiles the given files of iwae_amd/csrc -- default: kernels.hip row_kernels.hip wgrad_kernels.hip update_kernels.hip -- to /tmp/iwae_k_<file>.s once per call)"""
import collections, os, re, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pat, minm = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1
s = ""
for f in sys.argv[3:] or ["kernels.hip", "row_kernels.hip", "wgrad_kernels.hip", "update_kernels.hip"]:
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                           "-o", "/tmp/iwae_k_%s.s" % f, os.path.join(root, "iwae_amd", "csrc", f)], stderr=subprocess.DEVNULL)
    s += open("/tmp/iwae_k_%s.s" % f).read()
for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\s*s_endpgm", s, re.S | re.M):
    if pat not in m.group(1):
        continue
    print("==", m.group(1))
    parts = re.split(r"\n(\.LBB\d+_\d+):", m.group(2))
    blocks = [("entry", parts[0])] + [(parts[i], parts[i + 1]) for i in range(1, len(parts), 2)]
    for lab, b in blocks:
        ins = [l.strip().split()[0] for l in b.split("\n") if l.strip() and not l.strip().startswith((";", "."))]
        c = collections.Counter()
        for x in ins:
            c["mfma" if x.startswith("v_mfma") else "valu" if x.startswith("v_") else "salu" if x.startswith("s_") else
              "lds" if x.startswith("ds_") else "vmem" if x.startswith(("global_", "buffer_", "scratch_")) else "other"] += 1
        if c["mfma"] >= minm:
            print(lab, dict(c))
            print("    ", collections.Counter(x for x in ins if x.startswith("v_") and not x.startswith("v_mfma")).most_common(16))
