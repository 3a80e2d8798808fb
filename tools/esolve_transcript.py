"""Record what the eigensolvers print: tests/golden/esolve_transcript.json, case name -> list of lines, which tests/test_esolve_transcript_gpu.py replays.
    python tools/esolve_transcript.py [OUT.json]
The cases, the capture of the process's stdout at file-descriptor level and the masking of the `elapsed time` figures are tests/esolve_transcript_cases.py's:
the tool and the test run one list through one function.  Needs a HIP device.  Record on the commit whose text is to be held, BEFORE changing a print."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import esolve_transcript_cases as tc  # noqa: E402
import lis_amd  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    lib = lis_amd.load()
    if not lis_amd.gpu_available():
        raise SystemExit("esolve_transcript: no HIP device -- the eigensolvers have no CPU path")
    assert lib.initialize([]) == 0
    lib.dll.lis_amd_set_residency(0)
    doc = {}
    for name in tc.NAMES:
        err, lines = tc.replay(lib, name)
        assert err == 0, (name, err, lines[-5:])
        doc[name] = lines
        print(name, len(lines), "lines")
    with open(out, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
