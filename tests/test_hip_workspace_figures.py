"""mvlpt_text_workspace_bytes stays where it was (-m gpu; no kernel is launched).

The Python chunk planners compare the published figure with budgets (images_per_chunk, plan_text_chunks), so it is pinned, to the
byte, to tests/golden/text_workspace_bytes.json, which tools/make_workspace_golden.py recorded with the library of the commit
before the engine began to size its workspaces by their carve (the file names that library)."""
import itertools
import json
import os

import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# the grid, spelled out here as well: the golden file must hold exactly these figures, in this order (the last axis fastest)
AXES = {
    "C": [1, 3, 5, 1000],
    "L": [3, 20, 77],
    "save": [0, 1],
    "precision": ["fast", "split_grad"],
    "activation": ["quick_gelu", "gelu"],
    "act_ckpt": [1, 2, 3, 5, 12],
}
ARCH_NAMES = ["tiny", "ckpt128", "ViT-B/16", "ViT-H/14"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "text_workspace_bytes.json")) as f:
        return json.load(f)


def _arch(name):
    from mvlpt_amd.weights import ARCHS, WIDE_HEAD_ARCHS, ClipArch
    if name == "ckpt128":      # the 5-layer text tower of test_hip_act_ckpt.py's `small` fixture
        return ClipArch("ckpt128", 128, 32, 2, 128, 16, 77, 49408, 128, 2, 5)
    return WIDE_HEAD_ARCHS[name] if name in WIDE_HEAD_ARCHS else ARCHS[name]


def test_the_golden_file_holds_the_whole_grid(golden):
    assert golden["axes"] == AXES
    assert sorted(golden["bytes"]) == sorted(ARCH_NAMES)
    n = 1
    for v in AXES.values():
        n *= len(v)
    assert all(len(golden["bytes"][a]) == n for a in ARCH_NAMES)


@pytest.mark.parametrize("name", ARCH_NAMES)
def test_text_workspace_bytes_is_byte_identical(golden, name):
    from mvlpt_amd.engine import Engine
    want = golden["bytes"][name]
    eng = Engine(_arch(name), device=DEV)                # no weights: nothing is launched
    got = []
    try:
        for C_, L, save, prec, act, k in itertools.product(*AXES.values()):
            eng.set_precision(prec)
            eng.set_activation(act)
            eng.set_text_act_ckpt(k)
            got.append(eng.text_workspace_bytes(C_, L, bool(save)))
    finally:
        eng.set_precision("split_grad")
        eng.set_activation("quick_gelu")
        eng.set_text_act_ckpt(1)
    assert len(got) == len(want)
    for point, g, w in zip(itertools.product(*AXES.values()), got, want):
        assert g == w, f"{name} {dict(zip(AXES, point))}: {g} bytes, the golden file has {w}"
    eng.close()
