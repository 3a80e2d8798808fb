"""What the eigensolvers print at -eprint all, line for line: every served solver once (tests/esolve_transcript_cases.py), replayed under
lis_amd_set_reference_reductions(1) and compared with tests/golden/esolve_transcript.json, which tools/esolve_transcript.py recorded from this library
before its loops were merged into shared frames (host/lis_eloop.h, lis_esolver_single.c, lis_esolver_multi.c).  Only the figure after `elapsed time` is masked:
banners, labels and their padding, the iteration lines, the Ritz values, the per-mode reports of the refinements and the status line are all held."""
import json

import pytest

import esolve_transcript_cases as tc
import lis_amd

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(tc.GOLDEN))


@pytest.fixture(scope="module")
def lib():
    lib = lis_amd.load()
    assert lis_amd.gpu_available(), "no HIP device: the product path has no CPU fallback"
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    yield lib
    lib.dll.lis_amd_set_reference_reductions(0)


def test_the_golden_holds_exactly_the_shared_cases():
    assert sorted(GOLDEN) == sorted(tc.NAMES)


@pytest.mark.parametrize("name", tc.NAMES)
def test_the_printed_text_is_the_recorded_text(lib, name):
    err, lines = tc.replay(lib, name)
    assert err == 0, (name, err)
    want = GOLDEN[name]
    for k, (a, b) in enumerate(zip(lines, want)):
        assert a == b, (name, "line", k, a, b)
    assert len(lines) == len(want), (name, len(lines), len(want), lines[len(want):], want[len(lines):])
