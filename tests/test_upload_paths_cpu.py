"""The two builders of a matrix's HBM copy -- lisd_mat_ready / mat_upload (lis_amd/csrc/host/lis_upload.c) from host arrays, lisd_convert_csr
(lis_convert_hbm.c) from a CSR copy in HBM -- without a GPU: both files are compiled with gcc against stubs of everything they call (tests/c/upload_stubs.c),
tests/c/upload_cases.c runs them over a 6 x 6 bidiagonal matrix in every format, and every call sequence is held to the one written out here.

The sequences were written down from mat_upload, try_row_form, try_bsr_row_form and the five arms of lisd_convert_csr as they stood in lis_device.c, branch
by branch, not from the builders.  A token is the stub's short name and its scalar arguments: malloc(bytes), h2d / d2h / d2d(bytes), lazy(bytes,own=..).
One place differs from that code on a path that succeeds: where the DIA conversion tries the row form and drops it, the row counts' buffer is freed after
the dropped plan and rows instead of before them (conv_dia_dropped; the same calls, two releases in another order).

THE FAILURE SWEEP.  For every conversion case and every upload case that tries the row form, each position of the sequence whose stub can fail is made to
fail once: an allocation answers HIP code 2, lisp_alloc_lazy NULL, every other call 700.  A token marked `?` here is a call whose failure the code absorbs
(the result is still the form the case has without the failure), `?n` one whose failure costs the row form only (the conversion or upload still succeeds,
with the NATIVE form: an optimisation that runs out of memory is not an error).  A failure at any other position must come back as an error, with *done
still 0 and an EMPTY device record on the target.  After every run the copies are destroyed and nothing may be left alive: no device allocation, no plan,
no lazy host array; a free of something that is not live aborts the program.  Run against the code as it stood, the same sweep leaves something alive at
47 positions: a failing copy in up_i / up_d (the buffer just allocated), a failing csr_to_ell / csr_to_ell_rows launch, and every failing lisp_alloc_lazy
of the ELL, DIA, CSC and JAD arms.  Three things differ on purpose from that code on the failing paths: those buffers and pages are released; the
target's device record is empty after a failed conversion; and liship_ell_encode_indices answering anything but out-of-memory during an ELL conversion is
an error, as the upload always had it (it was swallowed)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis_amd", "csrc", "host")

PLAN6 = "plan(6) enc_idx enc_pat enc_val band"
PLAN2 = "plan(2) enc_idx enc_pat enc_val band"
DROP = "destroy free free free"                                      # the plan and the three arrays of a row form that found no value records
ROWS6_11 = "malloc(44) h2d(28) malloc(60) h2d(44) malloc(104) h2d(88)"          # up_i: (count + 4) ints, up_d: (count + 2) doubles; 7 / 11 / 11 entries
ROWS6_12 = "malloc(44) h2d(28) malloc(64) h2d(48) malloc(112) h2d(96)"          # the ELL row form: 6 rows of 2 slots
ROWS_TRY_11 = "malloc(44)?n h2d(28) malloc(60)?n h2d(44) malloc(104)?n h2d(88)"
ROWS_TRY_12 = "malloc(44)?n h2d(28) malloc(64)?n h2d(48) malloc(112)?n h2d(96)"
ELL_NATIVE = "malloc(64) h2d(48) malloc(112) h2d(96) ell_codes(6,2) ell_band(6,2)?"
DIA_NATIVE = "malloc(24) h2d(8) malloc(112) h2d(96)"
BSR_NATIVE = "malloc(32) h2d(16) malloc(36) h2d(20) malloc(176) h2d(160)"
BSR_TRY = "malloc(44)?n malloc(96)?n malloc(176)?n bsr_to_rows(6,2,2)"        # rptr n + 5 ints, 20 slots + 4 ints, 20 + 2 doubles
SPLIT2 = "malloc(28) h2d(12) malloc(24) h2d(8) malloc(32) h2d(16) sync"        # lis_split.c's rows (the stub: 2 rows, 2 entries)
SPLIT6 = "malloc(44) h2d(28) malloc(24) h2d(8) malloc(32) h2d(16) sync"        # a half of a split JAD matrix: 6 rows, 2 entries


def up(body, arrays):
    return f"init fill {body} sync" + " adopt" * arrays + " protect"


GATE = "malloc(8) row_facts(6) d2h(8) sync free"
FEW = "d2h(88)?n sync?n"                                             # the head of value[] for the few-distinct-values screen: cannot be read = not few
TAIL = "sync assemble"
ELL0 = f"{GATE} malloc(48) malloc(96) to_ell(6,2) {FEW}"
ELL_TRY = "malloc(28)?n malloc(48)?n malloc(96)?n to_ell_rows(6,2)"
DIA0 = f"{GATE} malloc(48) malloc(52) malloc(32) dia_offsets(6,6) malloc(8) malloc(96) to_dia(6,6,2) sync? free free {FEW}"
DIA_TRY = "malloc(24)?n malloc(28)?n dia_counts(6,6,2)?n malloc(44)?n malloc(88)?n dia_to_rows(6,6,2)?n"      # (whatever refuses on the way leaves the native form)
DIA_PLANE = "d2h(8)? sync?"                                          # the offsets, for the plane of the native kernels
CLONE = "malloc(28) malloc(44) malloc(88) d2d(28) d2d(44) d2d(88)"
BSR0 = f"{GATE} malloc(16) malloc(16) malloc(32) bsr_count(6,6,2,2) free free malloc(20) malloc(160) to_bsr(6,2,2,5) {FEW}"


def lazy(own, *sizes):
    return " ".join(f"lazy({b},own={own})" for b in sizes)


# name: (sequence, ret, done, type of the copy, pad_comm)
EXPECTED = {
    "up_csr": (up(f"{ROWS6_11} {PLAN6}", 3), 0, 0, "CSR", 0),
    "up_csc": (up(f"{ROWS6_11} sync {PLAN6}", 3), 0, 0, "CSR", 0),
    "up_jad": (up(f"{ROWS6_11} sync {PLAN6}", 4), 0, 0, "CSR", 0),
    "up_bsr": (up(BSR_NATIVE, 3), 0, 0, "BSR", 0),
    "up_split_csr": (up(f"split_rows {SPLIT2} {PLAN2} first_term(1)", 0), 0, 0, "CSR", 0),
    "up_split_jad": (up(f"split_jad_part(0) {SPLIT6} {PLAN6} split_jad_part(1) {SPLIT6} {PLAN6} malloc(64) h2d(48) malloc(176)", 0), 0, 0, "CSR", 0),
    "up_ell_native": (up(ELL_NATIVE, 2), 0, 0, "ELL", 0),
    "up_ell_codes_oom": (up(ELL_NATIVE, 2), 0, 0, "ELL", 0),
    "up_ell_rowform": (up(f"{ROWS_TRY_12} sync {PLAN6}", 2), 0, 0, "CSR", 0),
    "up_ell_dropped": (up(f"{ROWS_TRY_12} sync {PLAN6} {DROP} {ELL_NATIVE}", 2), 0, 0, "ELL", 0),
    "up_dia_native": (up(DIA_NATIVE, 2), 0, 0, "DIA", 0),
    "up_dia_rowform": (up(f"{ROWS_TRY_11} sync {PLAN6}", 2), 0, 0, "CSR", 0),
    "up_dia_dropped": (up(f"{ROWS_TRY_11} sync {PLAN6} {DROP} {DIA_NATIVE}", 2), 0, 0, "DIA", 0),
    "up_bsr_rowform": (up(f"{BSR_NATIVE} {BSR_TRY} {PLAN6} free free free", 3), 0, 0, "CSR", 0),          # the native arrays go
    "up_bsr_rowform_wide": (up(f"{BSR_NATIVE} {BSR_TRY} {PLAN6} enc_blk(2)? free free free", 3), 0, 0, "CSR", 0),
    "up_bsr_dropped": (up(f"{BSR_NATIVE} {BSR_TRY} {PLAN6} {DROP}", 3), 0, 0, "BSR", 0),
    "conv_ell_rowform": (f"{ELL0} {ELL_TRY} {PLAN6} {lazy(1, 48, 96)} set_ell(2) {TAIL}", 0, 1, "CSR", 0),
    "conv_ell_dropped": (f"{ELL0} {ELL_TRY} {PLAN6} {DROP} ell_codes(6,2) ell_band(6,2)? {lazy(0, 48, 96)} set_ell(2) {TAIL}", 0, 1, "ELL", 0),
    "conv_ell_native": (f"{ELL0} ell_codes(6,2) ell_band(6,2)? {lazy(0, 48, 96)} set_ell(2) {TAIL}", 0, 1, "ELL", 0),
    "conv_dia_rowform": (f"{DIA0} {DIA_TRY} {PLAN6} free free {lazy(1, 8, 96)} set_dia(2) {TAIL}", 0, 1, "CSR", 0),
    "conv_dia_dropped": (f"{DIA0} {DIA_TRY} {PLAN6} {DROP} free free {DIA_PLANE} {lazy(0, 8, 96)} set_dia(2) {TAIL}", 0, 1, "DIA", 0),
    "conv_dia_native": (f"{DIA0} free {DIA_PLANE} {lazy(0, 8, 96)} set_dia(2) {TAIL}", 0, 1, "DIA", 0),
    "conv_csc": (f"{GATE} malloc(28) malloc(44) malloc(88) malloc(84) transpose(6,6,11) sync free {CLONE} {PLAN6} {lazy(1, 28, 44, 88)} set_csc(11) {TAIL}", 0, 1, "CSR", 0),
    "conv_jad": (f"{GATE} jad_order malloc(24) malloc(12) malloc(44) malloc(88) h2d(24) h2d(12) to_jad(6) {CLONE} sync free free {PLAN6} {lazy(1, 44, 88)} "
                 f"set_jad(11,2) {TAIL}", 0, 1, "CSR", 0),
    "conv_bsr_rowform": (f"{BSR0} {BSR_TRY} {PLAN6} {lazy(1, 16, 20, 160)} set_bsr(2,2,5) {TAIL}", 0, 1, "CSR", 0),
    "conv_bsr_rowform_wide": (f"{BSR0} {BSR_TRY} {PLAN6} enc_blk(2)? {lazy(1, 16, 20, 160)} set_bsr(2,2,5) {TAIL}", 0, 1, "CSR", 0),
    "conv_bsr_dropped": (f"{BSR0} {BSR_TRY} {PLAN6} {DROP} {lazy(0, 16, 20, 160)} set_bsr(2,2,5) {TAIL}", 0, 1, "BSR", 0),
    "conv_bsr_native": (f"{BSR0} {lazy(0, 16, 20, 160)} set_bsr(2,2,5) {TAIL}", 0, 1, "BSR", 0),
    # 4 x 4 blocks on 6 rows: padding, so no row-form attempt (not even the screen), and pad_comm is set
    "conv_bsr_padding": (f"{GATE} malloc(12) malloc(12) malloc(32) bsr_count(6,6,4,4) free free malloc(20) malloc(640) to_bsr(6,4,4,5) {lazy(0, 12, 20, 640)} "
                         f"set_bsr(4,4,5) {TAIL}", 0, 1, "BSR", 2),
    # ---- not a case for the conversion in HBM
    "not_wrong_target": ("", 0, 0, "0", 0),
    "not_switched_off": ("", 0, 0, "0", 0),
    "not_two_ranks": ("", 0, 0, "0", 0),
    "not_split_source": ("", 0, 0, "0", 0),
    "not_ghost_columns": ("", 0, 0, "0", 0),
    "not_empty": ("", 0, 0, "0", 0),
    "not_device_only_jad": ("", 0, 0, "0", 0),
    "not_unsorted_dia": (GATE, 0, 0, "0", 0),
    "not_unsorted_csc": (GATE, 0, 0, "0", 0),
    "not_ell_too_wide": (GATE, 0, 0, "0", 0),                         # 6 rows of 357913942 slots: past 2^31 - 1
    "not_dia_none": (f"{GATE} malloc(48) malloc(52) malloc(32) dia_offsets(6,6) free free free", 0, 0, "0", 0),
    "not_bsr_none": (f"{GATE} malloc(16) malloc(16) malloc(32) bsr_count(6,6,2,2) free free free", 0, 0, "0", 0),
    "not_bsr_no_block_size": (GATE, 0, 0, "0", 0),
}
SWEPT = sorted(n for n in EXPECTED if n.startswith(("conv_", "not_")) or n in ("up_ell_rowform", "up_ell_dropped", "up_dia_rowform", "up_dia_dropped",
                                                                              "up_bsr_rowform", "up_bsr_rowform_wide", "up_bsr_dropped"))
NEVER_FAILS = {"free", "destroy", "trim", "init", "fill", "adopt", "protect", "release", "assemble", "jad_order", "split_rows", "split_jad_part", "storage_destroy",
               "hip_error", "lis_error", "set_ell", "set_dia", "set_csc", "set_jad", "set_bsr"}
NATIVE = {"up_ell": "ELL", "up_dia": "DIA", "up_bsr": "BSR", "conv_ell": "ELL", "conv_dia": "DIA", "conv_bsr": "BSR"}


def plain(sequence):
    return " ".join(t.rstrip("n").rstrip("?") if "?" in t else t for t in sequence.split())


def fallible(sequence):
    """(position, token, mark) of every call of the sequence that can fail"""
    out = []
    for pos, tok in enumerate(sequence.split()):
        mark = "?n" if tok.endswith("?n") else "?" if tok.endswith("?") else ""
        tok = tok[:len(tok) - len(mark)]
        if tok.split("(")[0] not in NEVER_FAILS:
            out.append((pos, tok, mark))
    return out


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upload_paths") / "upload_cases")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-I" + os.path.join(ROOT, "include"),
                    "-I" + HOST, os.path.join(HOST, "lis_upload.c"), os.path.join(HOST, "lis_convert_hbm.c"), os.path.join(ROOT, "tests", "c", "upload_stubs.c"),
                    os.path.join(ROOT, "tests", "c", "upload_cases.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout
    cases, sweep = {}, {}
    for line in out.splitlines():
        fields = [f.strip() for f in line.split("|")]
        if fields[0].startswith("sweep "):
            pos, tok = fields[1].split()
            answer = dict(f.split("=") for f in fields[2].split())
            sweep.setdefault(fields[0].split()[1], []).append((int(pos), tok, int(answer["ret"]), int(answer["done"]), answer["type"], fields[3]))
        else:
            answer = dict(f.split("=") for f in fields[2].split())
            assert fields[0] not in cases
            cases[fields[0]] = (fields[1], int(answer["ret"]), int(answer["done"]), answer["type"], int(answer["pad"]))
    return cases, sweep


def test_every_case_ran_and_every_case_is_expected(output):
    cases, sweep = output
    assert sorted(cases) == sorted(EXPECTED)
    assert sorted(sweep) == [n for n in SWEPT if fallible(EXPECTED[n][0])]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_call_sequence(output, name):
    sequence, ret, done, kind, pad = EXPECTED[name]
    assert output[0][name] == (plain(sequence), ret, done, kind, pad)


@pytest.mark.parametrize("name", [n for n in SWEPT if fallible(EXPECTED[n][0])])
def test_failure_sweep(output, name):
    sequence, _, done, kind, _ = EXPECTED[name]
    want = fallible(sequence)
    got = output[1][name]
    assert [(pos, tok) for pos, tok, *_ in got] == [(pos, tok) for pos, tok, _ in want]          # one line per fallible hit: a shortened sweep cannot pass
    for (pos, tok, mark), (_, _, ret, got_done, got_kind, state) in zip(want, got):
        where = f"{name}: position {pos}, {tok}"
        assert state == "clean", where
        if mark:                                  # absorbed: the same form, or the native one where the failure costs the row form
            assert (ret, got_done) == (0, done), where
            assert got_kind == (NATIVE["_".join(name.split("_")[:2])] if mark == "?n" else kind), where
        else:                                     # an error, and nothing of the target left
            assert ret != 0 and got_done == 0 and got_kind == "0", where
