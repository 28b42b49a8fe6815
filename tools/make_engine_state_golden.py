"""Record what a build of the library answers to the call sequences of tests/test_hip_engine_state.py (needs a GPU):

    MVLPT_HIP_LIB=<libmvlpt_hip.so of the build to record> python tools/make_engine_state_golden.py [out.json]

Writes tests/golden/engine_call_sequences.json: per sequence, [call, return code, error text] of every call.  The committed file was
recorded from the build in front of the engine's run records (csrc/engine.hip `Phase`), so the test holds the records to the
behaviour they replaced.  Only RECORDED sequences are run: on that build the BY_DESIGN ones run a backward over buffers no forward
has written, and what they should answer is written down in the test instead."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_hip_engine_state import GOLDEN, RECORDED, run_sequence  # noqa: E402


def main():
    from mvlpt_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    print("recording", _lib.LIB_PATH, _lib.lib.mvlpt_version().decode())
    golden = {}
    for name, (make_rig, steps) in RECORDED.items():
        golden[name] = run_sequence(make_rig(), steps)
        for call, rc, err in golden[name]:
            print(f"{name}: {call} -> {rc} {err}")
    with open(out, "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
