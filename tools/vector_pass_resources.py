"""Registers, scratch, LDS and occupancy of every kernel of kernels/vector_ops.hip and kernels/eigen.hip, of this tree beside another checkout (the
parent commit), from hipcc's -Rpass-analysis=kernel-resource-usage with the Makefile's flags.  No GPU is needed.  Prints the table kept in
profiles/vector_pass_resources.txt and exits non-zero when a kernel of this tree uses scratch or has a lower occupancy than the same kernel there.
    python tools/vector_pass_resources.py PARENT_CHECKOUT > profiles/vector_pass_resources.txt"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")
FILES = ["vector_ops.hip", "eigen.hip"]
FIELDS = [("VGPRs", "VGPRs"), ("SGPRs", "TotalSGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("LDS", r"LDS Size \[bytes/block\]"),
          ("occ", r"Occupancy \[waves/SIMD\]")]


def resources(root, name):
    """-> {demangled kernel: {field: int}}"""
    csrc = os.path.join(root, "lis_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall",
               "-Wno-unused-function", "-I" + os.path.join(root, "include"), "-Ikernels", "-Rpass-analysis=kernel-resource-usage",
               "-c", "kernels/" + name, "-o", os.path.join(tmp, "out.o")]
        text = subprocess.run(cmd, cwd=csrc, check=True, stderr=subprocess.PIPE, text=True).stderr
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, pat in FIELDS:
            m = re.search(r"remark:\s+" + pat + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    plain = subprocess.run(["c++filt"], input="\n".join(out), check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    short = lambda s: re.sub(r"\(.*$", "", s.replace("(anonymous namespace)::", "").replace("void ", ""))
    return {short(p): v for p, v in zip(plain, out.values())}


def main():
    parent = os.path.abspath(sys.argv[1])
    bad = []
    print("kernel resources, gfx950, the Makefile's flags: parent -> this tree   (VGPRs SGPRs scratch[B/lane] LDS[B/block] occupancy[waves/SIMD])")
    for name in FILES:
        old, new = resources(parent, name), resources(ROOT, name)
        print("\n%s: %d kernels at the parent, %d here" % (name, len(old), len(new)))
        for k in sorted(set(old) | set(new)):
            row = lambda r: "%3d %3d %3d %5d %d" % tuple(r[f] for f, _ in FIELDS) if r else "  -   -   -     - -"
            print("  %-72s %s  ->  %s" % (k, row(old.get(k)), row(new.get(k))))
            if k in new and (new[k]["scratch"] or (k in old and new[k]["occ"] < old[k]["occ"])):
                bad.append(k)
    print("\nkernels with scratch or a lower occupancy than at the parent: %s" % (", ".join(bad) if bad else "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
