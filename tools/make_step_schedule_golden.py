"""Record the step schedule of a Python tree for tests/test_hip_step_schedule.py (needs a GPU):

    python tools/make_step_schedule_golden.py [--package-root DIR] [out.json]

Writes tests/golden/step_schedule.json: per scenario the log of engine / stream / event calls, the sha256 of every step's loss and of
every prompt parameter after the last step.  DIR holds the `mvlpt_amd` package to record (default: this tree's); the scenarios and the
recorder are this tree's tests either way, and MVLPT_HIP_LIB names the library when DIR has none.  The committed file was recorded
from the tree in front of mvlpt_amd/schedule.py, on the same library, so the test holds that module to the schedule it replaced."""
import argparse
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=None)
    ap.add_argument("out", nargs="?", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    import mvlpt_amd
    from mvlpt_amd import _lib
    from tests.test_hip_step_schedule import GOLDEN, SCENARIOS, record
    print("recording", os.path.dirname(mvlpt_amd.__file__), _lib.LIB_PATH, _lib.lib.mvlpt_version().decode())
    golden = {}
    for name in SCENARIOS:
        with tempfile.TemporaryDirectory() as tmp:
            golden[name] = record(name, pathlib.Path(tmp))
        print(f"{name}: {len(golden[name]['log'])} calls, {len(golden[name]['losses'])} steps")
    out = args.out or GOLDEN
    with open(out, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
