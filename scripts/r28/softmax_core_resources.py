"""The compiler's resource report of every instance of the four attention kernels, parent against result, side by side.

    python scripts/r28/softmax_core_resources.py PARENT_TREE > profiles/r28/softmax_core_resources.txt

PARENT_TREE: a checkout of the parent commit (its graph-learn_amd/ and include/).  Compiles the three files for gfx950
with the Makefile's flags and -Rpass-analysis=kernel-resource-usage; needs no GPU."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FILES = ["glx_segment_softmax", "glx_gat_attention", "glx_dot_attention"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fvisibility=hidden", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage"]
FIELDS = [("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]


def report(tree, name, tmp):
    """{demangled kernel instance: {field: value}} of one file of one tree"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(tree, "graph-learn_amd", "csrc", name + ".hip")
    cmd = [hipcc] + FLAGS + ["-I" + os.path.join(tree, "include"), "-I" + os.path.dirname(src), "-c", src, "-o",
                             os.path.join(tmp, "x.o")]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, text=True, check=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = subprocess.run(["c++filt"] + list(out), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {re.sub(r"\(anonymous namespace\)::|\(.*", "", d).replace("void ", ""): out[k] for k, d in zip(out, names)}


def main():
    parent = os.path.abspath(sys.argv[1])
    print("Kernel resources for gfx950, parent -> result (template arguments as in the source: G, FLAT, [DROP,] BWD;")
    print("G, VEC, SUB for the dot-product kernels).  A line ends in `same` when every figure is unchanged.\n")
    print("%-58s %-10s %-10s %-8s %-10s %s" % ("instance", "VGPRs", "SGPRs", "scratch", "LDS", "occupancy"))
    worse = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in FILES:
            a, b = report(parent, name, tmp), report(ROOT, name, tmp)
            assert sorted(a) == sorted(b), "the kernel instances differ"
            for inst in sorted(a):
                cols = ["%d -> %d" % (a[inst][k], b[inst][k]) for _, k in FIELDS]
                same = a[inst] == b[inst]
                print("%-58s %-10s %-10s %-8s %-10s %s%s" % (inst, *cols, "  same" if same else ""))
                if b[inst]["scratch"] != 0 or b[inst]["lds"] != a[inst]["lds"] or b[inst]["occ"] < a[inst]["occ"]:
                    worse.append(inst)
    print("\nscratch 0, LDS unchanged and occupancy not lower in every instance: %s" % ("no: %s" % worse if worse else "yes"))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
