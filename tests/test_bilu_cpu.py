"""tests/bilu_oracle.py (the model of the block ILU(k) on BSR storage: pattern, term order, factor, M^-1) held to the reference library
at ONE thread in a child process (bn 1, 2, 3; fill 0, 1, 2), to itself at 3 and 8 row blocks (the reference cannot be run there, see
bilu_cases), and to tests/golden/bilu_bits.npz; and the entry points of liblis_amd that need no GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bilu_cases
import bilu_oracle
import ilu_cases
import lis_amd
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bilu_bits.npz")
GOLDEN_CASES = (("p125", 3, 1), ("twice", 2, 0))          # (name, bn, fill): a padded last block with fill-in; a block column stored twice


def test_block_ilu_symbols_are_exported():
    dll = C.CDLL(lis_amd.LIB_PATH)
    for name in ("lis_amd_last_solve_ilu_block", "liship_bilu_factor_f64", "liship_bilu_sweep_f64", "liship_block_gather_f64"):
        assert hasattr(dll, name), name


def test_no_block_ilu_solve_reported_before_any_solve():
    out = subprocess.run([sys.executable, "-c", "import lis_amd; lib = lis_amd.load(); print(lib.dll.lis_amd_last_solve_ilu_block())"],
                         capture_output=True, text=True, check=True, cwd=os.path.dirname(HERE))
    assert out.stdout.strip() == "0"


_models = {}


def model(name, bn, fill, T=1):
    """(factor, psolve of bilu_cases.rhs) of the model, computed once"""
    key = (name, bn, fill, T)
    if key not in _models:
        bsr = bilu_cases.system(name, bn)
        f = bilu_oracle.factor(*bsr, fill, T)
        _models[key] = (f, bilu_oracle.psolve(f, bilu_cases.rhs(bsr[4]), T))
    return _models[key]


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
def test_model_is_the_reference_at_one_thread():
    """pattern and order of L and U, every bit of L, U, Dinv and psolve (NaN sign and payload included: both run on this CPU)"""
    jobs = [dict(kind="factor", name=name, bn=bn, fill=fill) for name in bilu_cases.NAMED for bn in bilu_cases.BNS for fill in bilu_cases.FILLS]
    bad = []
    for job, want in zip(jobs, bilu_cases.reference_jobs(jobs)):
        got, x = model(job["name"], job["bn"], job["fill"])
        for d in bilu_cases.factor_differences(got, want):
            bad.append((job["name"], job["bn"], job["fill"], d))
        if not bilu_cases.same_bits(x, want["psolve"]):
            bad.append((job["name"], job["bn"], job["fill"], "psolve"))
    assert bad == []


@pytest.mark.parametrize("T", [3, 8])
@pytest.mark.parametrize("bn", bilu_cases.BNS)
def test_model_at_T_blocks_is_the_model_on_each_diagonal_block(T, bn):
    """at T row blocks the factor and M^-1 b are, block by block, those of the T = 1 model on the diagonal sub-matrix of each range of
    LIS_GET_ISIE over the block rows"""
    for name in ("p125", "nonsym", "twice"):
        bsr = bilu_cases.system(name, bn)
        bptr, bindex, value, _, n = bsr
        nr, bs = len(bptr) - 1, bn * bn
        b = bilu_cases.rhs(n)
        for fill in (0, 2):
            f, x = model(name, bn, fill, T)
            for lo, hi in bilu_oracle.row_blocks(nr, T):
                if hi == lo:
                    continue
                sub_n = min(n, hi * bn) - lo * bn
                sub = bilu_oracle.submatrix(bptr, bindex, value, bn, lo, hi)
                g = bilu_oracle.factor(*sub, bn, sub_n, fill, 1)
                for part in ("L", "U"):
                    p, c, v = f[part]
                    assert np.array_equal(p[lo:hi + 1] - p[lo], g[part][0]), (name, fill, part)
                    assert np.array_equal(c[p[lo]:p[hi]] - lo, g[part][1]), (name, fill, part)
                    assert bilu_cases.same_bits(v[p[lo] * bs:p[hi] * bs], g[part][2]), (name, fill, part)
                assert bilu_cases.same_bits(f["D"][lo * bs:hi * bs], g["D"]), (name, fill)
                assert bilu_cases.same_bits(x[lo * bn:lo * bn + sub_n], bilu_oracle.psolve(g, b[lo * bn:lo * bn + sub_n], 1)), (name, fill)


def test_twice_matrix_is_what_it_says():
    for bn in bilu_cases.BNS:
        bptr, bindex, value, _, n = bilu_cases.system("twice", bn)
        rows = [bindex[bptr[i]:bptr[i + 1]].tolist() for i in range(len(bptr) - 1)]
        assert rows[6].count(2) == 2 and rows[3].count(7) == 2 and rows[5].count(5) == 2 and 4 not in rows[4]
        assert any(r != sorted(r) for r in rows) and n % bn == (1 if bn > 1 else 0)
        for fill in bilu_cases.FILLS:
            f, x = model("twice", bn, fill)
            assert np.isfinite(f["D"]).all() and np.isfinite(f["L"][2]).all() and np.isfinite(f["U"][2]).all() and np.isfinite(x).all()
            assert f["L"][1][f["L"][0][6]:f["L"][0][7]].tolist().count(2) == 2       # the block column held twice stays twice in the pattern


def test_block_size_one_is_the_point_ilu():
    """bn = 1: the block model's L and U are the point model's on the same pattern; D is 1 / pivot"""
    import ilu_cases
    import ilu_oracle
    ptr, idx, val = ilu_cases.system("nonsym")
    for fill in bilu_cases.FILLS:
        f, _ = model("nonsym", 1, fill)
        g = ilu_oracle.factor(*bilu_oracle.csr_to_bsr(ptr, idx, val, 1), fill)
        assert bilu_cases.factor_differences(f, g) == []


SPECIAL_PIVOTS = (0.0, -0.0, float("inf"), 5e-324, float("nan"))


def special_pivot_systems():
    """dense 3-row matrices with the special value as the first pivot (rows 1 and 2 scale by its inverse and are updated through
    it) and as the second (reached through an update of its own)"""
    for p in SPECIAL_PIVOTS:
        for at in (0, 1):
            val = np.array([4.0, -1.0, 0.5, -2.0, 3.0, 1.5, 0.25, -0.75, 5.0])
            val[4 * at] = p
            if at == 1:
                val[1] = 0.0                                                      # row 1's pivot stays what was stored: 3.0 -> p, minus l * 0.0
            yield (p, at), (np.array([0, 3, 6, 9], np.int32), np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], np.int32), val)


def test_block_size_one_is_the_point_model_in_every_bit():
    """the identity kernels/ilu.hip rests on: the point form is the block form at bn = 1.  On the CSR arrays as they are
    (unsorted rows, columns stored twice, a row without a diagonal entry), for every fill and row-block count: the same pattern in the
    same term order, every bit of L, U and D, every bit of M^-1 b; and the same through pivots of +0.0, -0.0, inf, a denormal and NaN
    (NaN sign and payload left out, as everywhere in this project)"""
    import ilu_oracle
    cases = [((name, fill, T), ilu_cases.system(name), fill, T, True) for name in ilu_cases.NAMED for fill in ilu_cases.FILLS for T in ilu_cases.THREADS]
    cases += [(tag, sys3, 0, 1, False) for tag, sys3 in special_pivot_systems()]
    assert len(cases) == len(ilu_cases.NAMED) * len(ilu_cases.FILLS) * len(ilu_cases.THREADS) + 2 * len(SPECIAL_PIVOTS)
    for tag, (ptr, idx, val), fill, T, payload in cases:
        n = len(ptr) - 1
        b = bilu_cases.rhs(n)
        with np.errstate(all="ignore"):
            point = ilu_oracle.factor(ptr, idx, val, fill, T)
            block = bilu_oracle.factor(ptr, idx, val, 1, n, fill, T)
            assert ilu_cases.factor_differences(block, point, payload) == [], tag
            assert ilu_cases.same_bits(bilu_oracle.psolve(block, b, T), ilu_oracle.psolve(point, b, T), payload), tag
    special = [ilu_oracle.factor(*sys3, 0, 1)["D"] for _, sys3 in special_pivot_systems()]
    assert any(np.isinf(d).any() for d in special) and any(np.isnan(d).any() for d in special)      # the special pivots did reach the factor


def test_ilu_kernels_are_the_ones_meant_and_keep_their_blocks_in_registers(tmp_path):
    """kernels/ilu.hip compiled to gfx950 assembly with the library's flags (csrc/Makefile, HIPFLAGS), its kernel metadata read: ONE
    factorisation (level and run kernel for bn = 1, 2, 3) that CSR and BSR storage share, block sweeps for bn = 2, 3 only (bn = 1 runs
    the sweeps of sptrsv.hip), one gather; and no kernel with more private memory than before the point and block forms were joined
    (factorisation 24 bytes at bn = 1, 2, none at bn = 3; sweeps and gather none): a bn = 3 block that leaves the registers shows here"""
    import re
    csrc = os.path.join(os.path.dirname(HERE), "lis_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    asm = str(tmp_path / "ilu.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(os.path.dirname(HERE), "include"),
                    "-I" + os.path.join(csrc, "kernels"), "--cuda-device-only", "-S", os.path.join(csrc, "kernels", "ilu.hip"), "-o", asm],
                   check=True, capture_output=True, text=True)
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(asm).read())
    sizes = {name: int(size) for name, size in meta}
    factor = {(k, bn): [s for name, s in sizes.items() if k in name and "FacRowsILi%dE" % bn in name] for k in ("level_kernel", "run_kernel") for bn in (1, 2, 3)}
    sweeps = {(k, bn, d): [s for name, s in sizes.items() if k in name and "BSweepRowsILi%dELb%dE" % (bn, d) in name]
              for k in ("level_kernel", "run_kernel") for bn in (2, 3) for d in (0, 1)}
    gather = [s for name, s in sizes.items() if "block_gather_kernel" in name]
    assert all(len(v) == 1 for v in factor.values()) and all(len(v) == 1 for v in sweeps.values()) and len(gather) == 1, sorted(sizes)
    assert len(sizes) == 6 + 8 + 1, sorted(sizes)
    print("ILU KERNELS private segment:", sizes)
    for (k, bn), (size,) in factor.items():
        assert size <= (24 if bn < 3 else 0), (k, bn, size)
    assert all(size == 0 for (size,) in sweeps.values()) and gather == [0], sizes


def test_model_factor_reproduces_A_on_its_pattern():
    """meaning, without the reference: (L + I)(D + U) agrees with A on A's blocks for ILU(0) of a Poisson matrix in 3 x 3 blocks"""
    bptr, bindex, value, bn, n = bilu_cases.system("p125", 3)
    nr, bs = len(bptr) - 1, 9
    f, _ = model("p125", 3, 0)
    N = nr * bn
    Lm, Um = np.eye(N), np.zeros((N, N))
    for i in range(nr):
        Um[i * bn:(i + 1) * bn, i * bn:(i + 1) * bn] = np.linalg.inv(f["D"][i * bs:(i + 1) * bs].reshape(bn, bn).T)
    for M, part in ((Lm, f["L"]), (Um, f["U"])):
        p, c, v = part
        for i in range(nr):
            for k in range(p[i], p[i + 1]):
                M[i * bn:(i + 1) * bn, c[k] * bn:(c[k] + 1) * bn] = v[k * bs:(k + 1) * bs].reshape(bn, bn).T
    P = Lm @ Um
    for i in range(nr):
        for k in range(bptr[i], bptr[i + 1]):
            want = value[k * bs:(k + 1) * bs].reshape(bn, bn).T.copy()
            if i == nr - 1 and bindex[k] == i:
                for r in range(n % bn, bn):
                    want[r, r] = 1.0                                                  # the padding's diagonal
            assert np.abs(P[i * bn:(i + 1) * bn, bindex[k] * bn:(bindex[k] + 1) * bn] - want).max() <= 1e-13 * 6.0, (i, int(bindex[k]))


def golden_entries(factor_and_psolve):
    out = {}
    for (name, bn, fill), (f, x) in factor_and_psolve.items():
        tag = "%s_bn%d_fill%d" % (name, bn, fill)
        for part in ("L", "U"):
            for q, what in enumerate(("ptr", "index", "value")):
                out["%s_%s_%s" % (tag, part, what)] = f[part][q]
        out[tag + "_D"], out[tag + "_psolve"] = f["D"], x
    return out


def golden_case(G, name, bn, fill):
    tag = "%s_bn%d_fill%d" % (name, bn, fill)
    f = {"L": tuple(G["%s_L_%s" % (tag, w)] for w in ("ptr", "index", "value")), "U": tuple(G["%s_U_%s" % (tag, w)] for w in ("ptr", "index", "value")), "D": G[tag + "_D"]}
    return f, G[tag + "_psolve"]


def test_golden_is_what_the_model_computes():
    G = np.load(GOLDEN)
    for name, bn, fill in GOLDEN_CASES:
        want, wx = golden_case(G, name, bn, fill)
        got, x = model(name, bn, fill)
        assert bilu_cases.factor_differences(got, want) == [] and bilu_cases.same_bits(x, wx), (name, bn, fill)


@pytest.mark.skipif(not os.path.exists(orc.REF_SO), reason="oracle/_ref not built")
def test_golden_is_what_the_reference_computes():
    G = np.load(GOLDEN)
    jobs = [dict(kind="factor", name=name, bn=bn, fill=fill) for name, bn, fill in GOLDEN_CASES]
    for job, got in zip(jobs, bilu_cases.reference_jobs(jobs)):
        want, wx = golden_case(G, job["name"], job["bn"], job["fill"])
        assert bilu_cases.factor_differences(got, want) == [] and bilu_cases.same_bits(got["psolve"], wx), job
