"""The vector passes of kernels/vector_ops.hip, this tree's library against another checkout's (the parent commit, built), entry by entry.
Prints ONE JSON object (a run on an MI355X belongs in profiles/vector_pass_ab.json).
    python tools/vector_pass_probe.py PARENT_CHECKOUT
Each library runs in a child process of its own, in the order parent, new, parent, new.  A child times every entry by device events at n = 256^3 and
n = 40 * 2^20 (above the non-temporal-load threshold): ten warm-ups, then median, 10th and 90th percentile of thirty.  An entry holds when both of the
new library's medians lie within the parent's slower median plus the spread between the parent's own two medians."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [256 ** 3, 40 << 20]
WARM, REPS = 10, 30


def child(root):
    sys.path[:0] = [root, os.path.join(root, "tools")]
    import lis_amd
    from lis_amd import DeviceArray as DA, check
    from esi_probe import Timer
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("vector_pass_probe: no HIP device -- nothing here is measured without one")
    timer = Timer(lib, None)
    work, res = DA(lib.liship_reduce_work_bytes() // 8, np.float64), DA.zeros(4, np.float64)
    # device scalars: small coefficients (the data stays finite over the repetitions), {sum r^2, theta} = {1, 0} (the Ritz tail leaves r as it is)
    coef, sums = DA.from_host(np.array([1e-9, -1e-9, 0.5, 1e-9])), DA.from_host(np.array([1.0, 0.0]))
    ca, cna, cb = coef.ptr, coef.ptr + 8, coef.ptr + 16
    out = {}
    for n in SIZES:
        host = np.random.default_rng(5).uniform(0.5, 1.0, n + 2)
        a, b, c, d, e = (DA.from_host(host) for _ in range(5))
        w = work.ptr
        entries = {
            "axpy": lambda: lib.liship_axpy_f64(n, 1e-9, a.ptr, b.ptr, None),
            "axpy_xpay": lambda: lib.liship_axpy_xpay_f64(n, 1e-9, a.ptr, c.ptr, 0.5, b.ptr, None),
            "pmul_xpay": lambda: lib.liship_pmul_xpay_f64(n, a.ptr, c.ptr, 0.25, b.ptr, None),
            "dot": lambda: lib.liship_dot_f64(n, a.ptr, b.ptr, res.ptr, w, None),
            "nrm2": lambda: lib.liship_nrm2_f64(n, a.ptr, res.ptr, w, None),
            "cg_update_jacobi": lambda: lib.liship_cg_update_jacobi_f64(n, 1e-9, a.ptr, b.ptr, c.ptr, d.ptr, e.ptr, res.ptr, w, None),
            "axpy_sumsq_dot": lambda: lib.liship_axpy_sumsq_dot_f64(n, 1e-9, a.ptr, b.ptr, c.ptr, res.ptr, w, None),
            "cg_direction_dev": lambda: lib.liship_cg_direction_dev_f64(n, ca, cb, a.ptr, c.ptr, b.ptr, d.ptr, None),
            "bicgstab_end_dev": lambda: lib.liship_bicgstab_end_dev_f64(n, ca, ca, cna, a.ptr, b.ptr, c.ptr, d.ptr, e.ptr, res.ptr, w, None),
            "mgs_step": lambda: lib.liship_mgs_step_f64(n, ca, a.ptr, b.ptr, c.ptr, res.ptr, w, None),
            "ritz_tail": lambda: lib.liship_ritz_tail_f64(n, sums.ptr, d.ptr, e.ptr, res.ptr, w, None),
            "axpy_8B_aligned": lambda: lib.liship_axpy_f64(n, 1e-9, a.ptr + 8, b.ptr + 8, None),
        }
        row = out[str(n)] = {}
        for name, fn in entries.items():
            ms = np.array([timer.time(lambda: check(fn())) for _ in range(WARM + REPS)][WARM:])
            row[name] = {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
                         "p90_ms": round(float(np.percentile(ms, 90)), 4)}
        for x in (a, b, c, d, e):
            x.free()
    name = (C.c_char * 128)()
    lib.dll.liship_device_name(name, 128)
    print(json.dumps({"device": name.value.decode(), "entries": out}))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    parent = os.path.abspath(sys.argv[1])
    runs = []
    for label, root in (("parent", parent), ("new", ROOT)) * 2:
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], check=True, stdout=subprocess.PIPE, text=True).stdout
        runs.append({"library": label, **json.loads(text.strip().splitlines()[-1])})
    verdict = {}
    for n in runs[0]["entries"]:
        for name in runs[0]["entries"][n]:
            med = {lab: [r["entries"][n][name]["median_ms"] for r in runs if r["library"] == lab] for lab in ("parent", "new")}
            spread = abs(med["parent"][0] - med["parent"][1])
            bound = max(med["parent"]) + spread
            verdict.setdefault(n, {})[name] = {"parent_medians_ms": med["parent"], "new_medians_ms": med["new"], "noise_ms": round(spread, 4),
                                               "bound_ms": round(bound, 4), "holds": bool(max(med["new"]) <= bound)}
    print(json.dumps({"tool": "tools/vector_pass_probe.py", "device": runs[0]["device"], "warmups": WARM, "samples": REPS, "order": [r["library"] for r in runs],
                      "runs": runs, "verdict": verdict}, indent=1))


if __name__ == "__main__":
    main()
