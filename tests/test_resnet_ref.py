"""CPU tests of the ResNet-backbone plumbing: the float64 restatement (tests/resnet_ref.py) against the fixtures of the REAL reference
(tools/make_resnet_golden.py), the feasibility of the 1e-3 tower bar under the device's fp16 rounding points, the weight generator,
the architecture tables and the argument validation of mvlpt_create_resnet."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from tests import resnet_ref as R
from tests.golden_util import GOLDEN, load_npz, t

FEATURE_CASES = [("tiny_rn_features", "", "tiny-rn", 0), ("tiny_rn_features", "r96_", "tiny-rn", 96),
                 ("full_rn50_features", "", "RN50", 0), ("full_rn101_features", "", "RN101", 0)]
IDS = ["tiny-rn", "tiny-rn-96", "RN50", "RN101"]


def case_inputs(fixture, prefix, arch_name, resolution):
    """(arch, state dict, image, fixture): weights and image regenerated from the fixture's seeds."""
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    z = load_npz(fixture)
    arch = RESNET_ARCHS[arch_name]
    if resolution:
        arch = dataclasses.replace(arch, image_resolution=resolution)
    assert int(z[prefix + "image_resolution"]) == arch.image_resolution
    sd = make_state_dict(arch, int(z[prefix + "weight_seed"]))
    g = torch.Generator().manual_seed(int(z[prefix + "image_seed"]))
    image = torch.randn(int(z[prefix + "image_batch"]), 3, arch.image_resolution, arch.image_resolution, generator=g)
    return arch, sd, image, {k[len(prefix):]: v for k, v in z.items() if k.startswith(prefix) and (prefix or not k.startswith("r96_"))}


@pytest.fixture(scope="module")
def restated():
    """float64 and fp16-emulated features of every fixture, computed once."""
    out = {}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for case, name in zip(FEATURE_CASES, IDS):
        arch, sd, image, z = case_inputs(*case)
        stages = {}
        exact = R.resnet_features(sd, image, arch.vision_layers, stages=stages)
        emulated = R.resnet_features(sd, image, arch.vision_layers, round16=True)
        out[name] = (z, exact, emulated, stages)
    return out


@pytest.mark.parametrize("name", IDS)
def test_restatement_matches_the_reference(name, restated):
    """The project's restatement tolerance (tests/test_oracle_golden.py: rtol 2e-4, atol scaled to the fixture): the fixture is the
    reference's fp32 CPU run, the restatement float64."""
    z, exact, _, stages = restated[name]
    ref = t(z["features"]).double()
    err = float((exact - ref).abs().max()) / float(ref.abs().max())
    print(f"{name}: restatement vs reference features {err:.3e} of max|ref|")
    assert torch.allclose(exact, ref, rtol=2e-4, atol=2e-4 * float(ref.abs().max()))
    for st in R.STAGES:
        for k in ("mean", "rms", "sample"):
            want = t(np.asarray(z[f"{st}_{k}"])).double()
            assert torch.allclose(stages[st][k], want, rtol=2e-4, atol=2e-4 * float(t(np.asarray(z[f"{st}_rms"])))), f"{st} {k}"


@pytest.mark.parametrize("name", IDS)
def test_fp16_rounding_points_leave_half_of_the_budget(name, restated):
    """The device rounds to fp16 where resnet_ref(round16=True) does.  With exact accumulation that alone must cost at most 0.5e-3 of
    max|feature|: the other half of the 1e-3 tower bar is left to the accumulation order."""
    z, exact, emulated, _ = restated[name]
    err = float((emulated - exact).abs().max()) / float(exact.abs().max())
    print(f"{name}: fp16 rounding points cost {err:.3e} of max|feature|")
    assert err <= 0.5e-3


def test_generator_emits_the_reference_keys_for_rn50():
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    with open(os.path.join(GOLDEN, "ref_rn50_keys.json")) as f:
        want = json.load(f)["state_dict"]
    sd = make_state_dict(RESNET_ARCHS["RN50"], 0, include_token_embedding=True)
    assert {k: list(v.shape) for k, v in sd.items()} == want
    assert sd["visual.bn1.num_batches_tracked"].dtype == torch.int64
    for k, v in sd.items():
        if k.endswith("conv1.weight") or k.endswith("_proj.weight"):
            assert torch.equal(v, v.half().float()), f"{k} must be fp16-exact"


def test_generator_keeps_rn101_blocks_in_fp16_range():
    """33 blocks deep: bn3's gain of 0.25 keeps the rms of every block output near 1 (0.5 lets it grow past 20, the reference's
    zero init would hide the residual branch)."""
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    arch = RESNET_ARCHS["RN101"]
    sd = make_state_dict(arch, 2)
    assert 0.2 < float(sd["visual.layer3.5.bn3.weight"].mean()) < 0.3
    rms = []
    image = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    R.resnet_features(sd, image, arch.vision_layers, block_rms=rms)
    assert len(rms) == 33
    print("RN101 block rms: min %.3f max %.3f" % (min(rms), max(rms)))
    assert 0.1 <= min(rms) and max(rms) <= 3.0


def test_arch_tables_and_lookup():
    from mvlpt_amd.weights import ARCHS, RESNET_ARCHS, arch_from_state_dict, get_arch, make_state_dict
    assert "RN50" not in ARCHS and "RN101" not in ARCHS and "tiny-rn" not in ARCHS
    assert sorted(ARCHS) == sorted(["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px", "tiny"])
    assert sorted(RESNET_ARCHS) == ["RN101", "RN50", "tiny-rn"]
    for name in list(ARCHS) + list(RESNET_ARCHS):
        assert get_arch(name).name == name
    with pytest.raises(KeyError):
        get_arch("RN50x4")
    rn50 = RESNET_ARCHS["RN50"]
    assert rn50.vision_heads == 32 and rn50.grid == 7 and rn50.ctor_args() == (1024, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12)
    assert RESNET_ARCHS["RN101"].ctor_args() == (512, 224, (3, 4, 23, 3), 64, None, 77, 49408, 512, 8, 12)
    tiny = RESNET_ARCHS["tiny-rn"]
    assert (tiny.embed_dim, tiny.image_resolution, tiny.vision_layers, tiny.vision_width, tiny.grid ** 2 + 1) == (128, 64, (1, 2, 1, 1), 16, 5)
    for name, arch in RESNET_ARCHS.items():
        assert arch_from_state_dict(make_state_dict(arch, 0), name) == arch
    assert arch_from_state_dict(make_state_dict(ARCHS["tiny"], 0), "tiny") == ARCHS["tiny"]


def test_create_resnet_validates_its_arguments_without_a_gpu():
    from mvlpt_amd import _lib
    lib = _lib.lib

    def create(text=(77, 128, 2, 2, 128, _lib.DT_F16), vit=(0, 0, 0, 0, 0), rn=(64, 16, (1, 2, 1, 1), 8, 128)):
        a = _lib.MvlptArch(*vit, *text)
        r = _lib.MvlptResNetArch(rn[0], rn[1], (C.c_int * 4)(*rn[2]), rn[3], rn[4])
        h = C.c_void_p()
        rc = lib.mvlpt_create_resnet(C.byref(a), C.byref(r), C.byref(h))
        if rc == 0:
            lib.mvlpt_destroy(h)
        return rc, _lib.last_error(None)

    assert lib.mvlpt_create_resnet(None, None, None) == _lib.ERR_ARG
    assert create(vit=(224, 0, 0, 0, 0))[0] == _lib.ERR_ARG                          # a ViT field set
    assert create(rn=(72, 16, (1, 2, 1, 1), 8, 128))[0] == _lib.ERR_ARG              # resolution % 32
    assert create(rn=(64, 18, (1, 2, 1, 1), 9, 128))[0] == _lib.ERR_ARG              # width % 4
    assert create(rn=(64, 16, (1, 2, 1, 1), 4, 128))[0] == _lib.ERR_ARG              # heads * 64 != 32 * width
    assert create(rn=(64, 16, (1, 2, 1, 1), 8, 256))[0] == _lib.ERR_ARG              # output_dim != embed_dim
    assert create(rn=(64, 16, (1, 0, 1, 1), 8, 128))[0] == _lib.ERR_ARG              # an empty stage
    rc, msg = create(text=(77, 128, 2, 2, 128, _lib.DT_BF16))
    assert rc == _lib.ERR_UNSUPPORTED and "fp16" in msg
    # everything valid: the only thing missing is the device (with one, the handle is created and destroyed again)
    rc, msg = create()
    assert rc in (0, _lib.ERR_HIP), msg
