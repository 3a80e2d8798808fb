"""What the eigensolvers print: the cases, the replay and the masking that tools/esolve_transcript.py (which records tests/golden/esolve_transcript.json) and
tests/test_esolve_transcript_gpu.py (which compares against it) share, so that the test replays exactly what the tool ran.

Each case is one lis_esolve / lis_gesolve with -eprint all under lis_amd_set_reference_reductions(1), tiny and cut short by -emaxiter 6: the text is what
is held, not convergence.  Every served solver appears once; `nonsym7 ai` is there for the complex-pair branch of Arnoldi's Ritz read-out."""
import ctypes as C
import os
import re
import sys
import tempfile

import esolve_drv
import gesolve_drv
import gesolve_multi_cases

COMMON = " -etol 1e-10 -emaxiter 6 -eprint all"
# (name, matrix or pencil, options, the caller's x is esolve_drv.start_vector)
CASES = [
    ("pi", "sym7", "-e pi", False),
    ("ii", "sym7", "-e ii", False),
    ("rqi", "sym7", "-e rqi -initx_ones false", True),
    ("cg", "sym7", "-e cg", False),
    ("cr", "sym7", "-e cr -shift 0.75", False),
    ("si", "sym7", "-e si -ss 3 -ie ii -shift 0.75", False),
    ("li", "sym7", "-e li -ss 3", False),
    ("ai", "sym7", "-e ai -ss 3 -ie rqi", False),
    ("ai_nonsym", "nonsym7", "-e ai -ss 4", False),
    ("gpi", "P1", "-e gpi", False),
    ("gii", "P1", "-e gii -shift 0.005", False),
    ("grqi", "P1", "-e grqi", False),
    ("gcr", "P1", "-e gcr", False),
    ("gsi", "P1", "-e gsi -ss 3 -ige gpi", False),
    ("gli", "P1", "-e gli -ss 3", False),
    ("gai", "P1", "-e gai -ss 3 -ige gcr", False),
]
NAMES = [c[0] for c in CASES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "esolve_transcript.json")
_ELAPSED = re.compile(r"(elapsed time\s*= )\S+")


def captured(fn):
    """(fn(), what the process wrote to file descriptor 1 while fn ran)"""
    libc = C.CDLL(None)
    sys.stdout.flush()
    libc.fflush(None)
    keep = os.dup(1)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 1)
        try:
            out = fn()
            libc.fflush(None)
        finally:
            os.dup2(keep, 1)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def masked(text):
    """the lines of a transcript with the one thing that differs from run to run -- the number after `elapsed time` -- replaced by a fixed token"""
    return [_ELAPSED.sub(r"\1<t>", line) for line in text.splitlines()]


def replay(lib, name):
    """-> (err, masked lines) of one case"""
    _, where, opts, given = CASES[NAMES.index(name)]
    if where in esolve_drv.MATRICES:
        A, B = esolve_drv.make_matrix(lib, where), None
    else:
        A, B = gesolve_multi_cases.make_pencil(lib, where)
    x0 = esolve_drv.start_vector(A.contents.n) if given else None
    assert lib.dll.lis_amd_set_reference_reductions(1) == 0
    try:
        if B is None:
            res, text = captured(lambda: esolve_drv.esolve(lib, A, opts + COMMON, x0))
        else:
            res, text = captured(lambda: gesolve_drv.gesolve(lib, A, B, opts + COMMON, x0))
    finally:
        lib.dll.lis_amd_set_reference_reductions(0)
    lib.lis_matrix_destroy(A)
    if B is not None:
        lib.lis_matrix_destroy(B)
    return res["err"], masked(text)
