"""The product dispatch (lis_amd/csrc/host/lis_product.c: lisd_spmv, lisd_spmv_dot_launch_to) without a GPU: the file is compiled with gcc against stubs of
everything it calls (tests/c/product_stubs.c), tests/c/product_cases.c runs it over hand-made matrix records, and every call sequence is held to the one
written out here.

The sequences were written down from the `if` chains this file replaced (lisd_spmv and lisd_spmv_dot_launch_to as they stood in lis_device.c), branch by
branch, not from the table.  Three places differ from those chains on purpose:
  * a split JAD matrix (d->type CSR, L in d->plan, U in d->u_plan) on a rank without ghost columns in a multi-rank job took the CSR row-range branch and
    returned L x; it has no row-range form, so it exchanges first and runs its four launches (split_jad_r2_no_ghosts*);
  * a row-range launcher launches nothing for an empty range and answers 0 (the stubs do the same), so the BSR branch's calls for an empty head or tail are
    not made any more (bsr_r2_no_head, bsr_r2_no_tail);
  * a hard error of the interior part of the plain product now ends the exchange before it fails, as the fused product always did (csr_r2_interior_error).
`served` counts the product once, and once more where the fused entry goes through lisd_spmv (the lazy renumbering waits for that count)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis_amd", "csrc", "host")

SPLIT = "csr(plan=1) pmul_xpay(40) csr(plan=2) axpy(40)"          # w = L x; w = D.*x + w; y = U x; y += w
STRIPS = "set_plane(0)"                                             # fmt_strips: in front of every whole-matrix ELL / DIA launch (40 rows: no plane)


def rows(fmt, b, e, end, extra=""):
    """interior under the halo, then head and tail behind it"""
    parts = [f"halo_begin {fmt}_rows({b},{e}{extra}) halo_end"]
    if b > 0:
        parts.append(f"{fmt}_rows(0,{b}{extra})")
    if e < end:
        parts.append(f"{fmt}_rows({e},{end}{extra})")
    return " ".join(parts)


NC = ",codes=0"
EXPECTED = {
    # ---- one rank
    "csr": ("csr(plan=1)", 1, 0),
    "csr_table_one_rank": ("csr(plan=1)", 1, 0),
    "ell": (f"{STRIPS} ell", 1, 0),
    "ell_codes": (f"{STRIPS} ell_coded(sq=-1)", 1, 0),
    "ell_codes_refused": (f"{STRIPS} ell_coded(sq=-1) ell", 1, 0),
    "ell_strips": ("set_plane(4096) ell", 1, 0),                   # x beyond 256 MB and a plane found at upload time
    "dia": (f"{STRIPS} dia", 1, 0),
    "jad": ("jad", 1, 0),
    "bsr": ("bsr_nnz", 1, 0),
    "split_jad": (SPLIT, 1, 0),
    "csr_error": ("csr(plan=1) hip_error(700)", 1, 77),
    "csr_dot": ("csr_dot(sq=0)", 1, 0),
    "csr_dot2": ("csr_dot(sq=1)", 1, 0),
    "csr_dot_refused": ("csr_dot(sq=0) csr(plan=1) dot(40)", 1, 0),
    "csr_dot_error": ("csr_dot(sq=0) hip_error(700)", 1, 77),
    "csr_dot_plan_not_fused": ("csr(plan=1) dot(40)", 2, 0),
    "csr_dot_fusion_off": ("csr(plan=1) dot(40)", 2, 0),
    "ell_dot": (f"{STRIPS} ell_dot(sq=0)", 1, 0),
    "ell_dot_codes": (f"{STRIPS} ell_coded(sq=0)", 1, 0),
    "ell_dot2_codes": (f"{STRIPS} ell_coded(sq=1)", 1, 0),
    "ell_dot_codes_refused": (f"{STRIPS} ell_coded(sq=0) ell dot(40)", 1, 0),          # straight to the 4-byte-index kernel, no strips again
    "ell_dot_refused": (f"{STRIPS} ell_dot(sq=0) ell dot(40)", 1, 0),
    "ell_dot_fusion_off": (f"{STRIPS} ell dot(40)", 2, 0),
    "ell_dot_codes_fusion_off": (f"{STRIPS} ell_coded(sq=-1) dot(40)", 2, 0),
    "dia_dot": (f"{STRIPS} dia_dot(sq=0)", 1, 0),
    "dia_dot_refused": (f"{STRIPS} dia_dot(sq=1) dia dot2(40)", 1, 0),
    "dia_dot_fusion_off": (f"{STRIPS} dia dot(40)", 2, 0),
    "jad_dot": ("jad dot(40)", 2, 0),
    "jad_dot2": ("jad dot2(40)", 2, 0),
    "bsr_dot": ("bsr_dot(sq=0)", 1, 0),
    "bsr_dot_refused": ("bsr_dot(sq=0) bsr_nnz dot(40)", 1, 0),
    "bsr_dot_blocks_not_square": ("bsr_nnz dot(40)", 2, 0),
    "bsr_dot_fusion_off": ("bsr_nnz dot(40)", 2, 0),
    "split_jad_dot": (f"{SPLIT} dot(40)", 2, 0),
    "split_jad_dot2": (f"{SPLIT} dot2(40)", 2, 0),
    # ---- two ranks, the plain product (40 rows; BSR: 20 block rows, and its threshold counts those)
    "csr_r2_both": (rows("csr", 5, 35, 40), 1, 0),
    "csr_r2_no_head": (rows("csr", 0, 30, 40), 1, 0),
    "csr_r2_no_tail": (rows("csr", 10, 40, 40), 1, 0),
    "csr_r2_half": (rows("csr", 20, 40, 40), 1, 0),
    "csr_r2_under_half": ("halo_device csr(plan=1)", 1, 0),
    "csr_r2_overlap_off": ("halo_device csr(plan=1)", 1, 0),
    "csr_r2_all_inner": ("halo_begin csr_rows(0,40) halo_end", 1, 0),
    "ell_r2_both": (rows("ell", 5, 35, 40, NC), 1, 0),
    "ell_r2_no_head": (rows("ell", 0, 30, 40, NC), 1, 0),
    "ell_r2_no_tail": (rows("ell", 10, 40, 40, NC), 1, 0),
    "ell_r2_under_half": (f"halo_device {STRIPS} ell", 1, 0),
    "ell_r2_overlap_off": (f"halo_device {STRIPS} ell", 1, 0),
    "ell_r2_codes": (rows("ell", 5, 35, 40, ",codes=1"), 1, 0),    # the row-range launcher takes the codes as arguments
    "ell_r2_codes_under_half": (f"halo_device {STRIPS} ell_coded(sq=-1)", 1, 0),
    "dia_r2_both": (rows("dia", 5, 35, 40), 1, 0),
    "dia_r2_no_head": (rows("dia", 0, 30, 40), 1, 0),
    "dia_r2_no_tail": (rows("dia", 10, 40, 40), 1, 0),
    "dia_r2_under_half": (f"halo_device {STRIPS} dia", 1, 0),
    "dia_r2_overlap_off": (f"halo_device {STRIPS} dia", 1, 0),
    "bsr_r2_both": (rows("bsr", 3, 17, 20), 1, 0),
    "bsr_r2_no_head": (rows("bsr", 0, 15, 20), 1, 0),
    "bsr_r2_no_tail": (rows("bsr", 5, 20, 20), 1, 0),
    "bsr_r2_half_of_block_rows": (rows("bsr", 0, 10, 20), 1, 0),   # 10 of 20 block rows; 10 of 40 rows would not do
    "bsr_r2_under_half": ("halo_device bsr_nnz", 1, 0),
    "bsr_r2_overlap_off": ("halo_device bsr_nnz", 1, 0),
    "jad_r2": ("halo_device jad", 1, 0),
    "split_jad_r2_no_ghosts": (f"halo_device {SPLIT}", 1, 0),
    "csr_r2_interior_error": ("halo_begin csr_rows(5,35) halo_end hip_error(-1)", 1, 77),
    # ---- two ranks, the fused product: in row ranges for CSR alone, and only when its partial sums (here one per row) all find a slot
    "csr_r2_dot_slots_fit": ("halo_begin csr_rows_dot(5,35,slot=0,sq=0) halo_end csr_rows_dot(0,5,slot=30,sq=0) csr_rows_dot(35,40,slot=35,sq=0) "
                             "csr_dot_finish(slots=40,sq=0)", 1, 0),
    "csr_r2_dot2_slots_fit": ("halo_begin csr_rows_dot(5,35,slot=0,sq=1) halo_end csr_rows_dot(0,5,slot=30,sq=1) csr_rows_dot(35,40,slot=35,sq=1) "
                              "csr_dot_finish(slots=40,sq=1)", 1, 0),
    "csr_r2_dot_slots_just_fit": ("halo_begin csr_rows_dot(5,35,slot=0,sq=0) halo_end csr_rows_dot(0,5,slot=30,sq=0) csr_rows_dot(35,40,slot=35,sq=0) "
                                  "csr_dot_finish(slots=40,sq=0)", 1, 0),
    "csr_r2_dot_no_head": ("halo_begin csr_rows_dot(0,30,slot=0,sq=0) halo_end csr_rows_dot(30,40,slot=30,sq=0) csr_dot_finish(slots=40,sq=0)", 1, 0),
    "csr_r2_dot_no_tail": ("halo_begin csr_rows_dot(10,40,slot=0,sq=0) halo_end csr_rows_dot(0,10,slot=30,sq=0) csr_dot_finish(slots=40,sq=0)", 1, 0),
    "csr_r2_dot_slots_do_not_fit": (rows("csr", 5, 35, 40) + " dot(40)", 2, 0),
    "csr_r2_dot_plan_not_fused": (rows("csr", 5, 35, 40) + " dot(40)", 2, 0),
    "csr_r2_dot_interior_refuses": ("halo_begin csr_rows_dot(5,35,slot=0,sq=0) halo_end csr(plan=1) dot(40)", 1, 0),      # the ghosts are in: no second exchange
    "csr_r2_dot_interior_error": ("halo_begin csr_rows_dot(5,35,slot=0,sq=0) halo_end hip_error(700)", 1, 77),
    "csr_r2_dot_fusion_off": (rows("csr", 5, 35, 40) + " dot(40)", 2, 0),
    "csr_r2_dot_under_half": ("halo_device csr_dot(sq=0)", 1, 0),
    "csr_r2_dot_overlap_off": ("halo_device csr_dot(sq=0)", 1, 0),
    "csr_r2_dot_under_half_refused": ("halo_device csr_dot(sq=0) csr(plan=1) dot(40)", 1, 0),
    "ell_r2_dot": (f"halo_device {STRIPS} ell_dot(sq=0)", 1, 0),   # ELL / DIA / BSR: exchange first, one launch
    "ell_r2_dot_refused": (f"halo_device {STRIPS} ell_dot(sq=0) ell dot(40)", 1, 0),
    "ell_r2_dot_fusion_off": (rows("ell", 5, 35, 40, NC) + " dot(40)", 2, 0),
    "dia_r2_dot": (f"halo_device {STRIPS} dia_dot(sq=0)", 1, 0),
    "dia_r2_dot_fusion_off": (rows("dia", 5, 35, 40) + " dot(40)", 2, 0),
    "bsr_r2_dot": ("halo_device bsr_dot(sq=0)", 1, 0),
    "bsr_r2_dot_blocks_not_square": (rows("bsr", 3, 17, 20) + " dot2(40)", 2, 0),
    "jad_r2_dot": ("halo_device jad dot(40)", 2, 0),
    "split_jad_r2_no_ghosts_dot": (f"halo_device {SPLIT} dot(40)", 2, 0),
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("product_dispatch") / "product_cases")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                    os.path.join(HOST, "lis_product.c"), os.path.join(ROOT, "tests", "c", "product_stubs.c"), os.path.join(ROOT, "tests", "c", "product_cases.c"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    got = {}
    for line in out.splitlines():
        name, log, tail = (f.strip() for f in line.split("|"))
        served, ret = (int(f.split("=")[1]) for f in tail.split())
        assert name not in got
        got[name] = (log, served, ret)
    return got


def test_every_case_ran_and_every_case_is_expected(lines):
    assert sorted(lines) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_launch_sequence(lines, name):
    assert lines[name] == EXPECTED[name]
