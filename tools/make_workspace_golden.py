"""Writes tests/golden/text_workspace_bytes.json: what mvlpt_text_workspace_bytes publishes over a grid of architectures, sequence
counts and lengths, save settings, precision modes, activations and activation-checkpointing settings.

The Python chunk planners compare the figure with budgets, so a change of the engine's workspace code must leave it where it is:
record the file with the library of the commit BEFORE such a change (build that commit elsewhere and select its library with
MVLPT_HIP_LIB), never with the code under test.  The library's own version string (source hash and commit) is stored in the file.
Engines are built without weights: nothing is launched.  Needs a HIP device (an Engine does).

Usage: MVLPT_HIP_LIB=/path/to/parent/libmvlpt_hip.so python tools/make_workspace_golden.py [out.json]"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "text_workspace_bytes.json")

# every axis in the order the figures are stored (itertools.product over them, the last one fastest)
AXES = {
    "C": [1, 3, 5, 1000],
    "L": [3, 20, 77],
    "save": [0, 1],
    "precision": ["fast", "split_grad"],
    "activation": ["quick_gelu", "gelu"],
    "act_ckpt": [1, 2, 3, 5, 12],
}


def archs():
    from mvlpt_amd.weights import ARCHS, WIDE_HEAD_ARCHS, ClipArch
    # "ckpt128": the 5-layer text tower of tests/test_hip_act_ckpt.py's `small` fixture
    return {"tiny": ARCHS["tiny"], "ckpt128": ClipArch("ckpt128", 128, 32, 2, 128, 16, 77, 49408, 128, 2, 5),
            "ViT-B/16": ARCHS["ViT-B/16"], "ViT-H/14": WIDE_HEAD_ARCHS["ViT-H/14"]}


def figures(eng):
    """The published figure at every grid point, in AXES order.  Leaves the engine's settings at their defaults."""
    out = []
    try:
        for C_, L, save, prec, act, k in itertools.product(*AXES.values()):
            eng.set_precision(prec)
            eng.set_activation(act)
            eng.set_text_act_ckpt(k)
            out.append(eng.text_workspace_bytes(C_, L, bool(save)))
    finally:
        eng.set_precision("split_grad")
        eng.set_activation("quick_gelu")
        eng.set_text_act_ckpt(1)
    return out


def main():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import Engine
    out = {"library": _lib.lib.mvlpt_version().decode(), "axes": AXES, "bytes": {}}
    for name, arch in archs().items():
        eng = Engine(arch)
        out["bytes"][name] = figures(eng)
        eng.close()
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {sum(len(v) for v in out['bytes'].values())} figures from {out['library']}")


if __name__ == "__main__":
    main()
