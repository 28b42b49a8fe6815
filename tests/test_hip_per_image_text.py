"""The per-image text towers' chunk planner on a live engine (-m gpu): the condition its equivalence with the former uniform planner
rests on (tests/test_per_image_text_host.py), and the exact chunk list under a budget of two images.  Rigs: the tiny CoCoOp fixture with
B = 7 of tests/test_hip_cocoop.py and the tiny TPT model of tests/test_hip_tpt.py."""
import pytest
import torch

from tests import tpt_path_ref as P
from tests.golden_util import load_npz
from tests.test_hip_cocoop import build_cocoop, run_cocoop
from tests.test_hip_tpt import DEV, make_cfg

pytestmark = pytest.mark.gpu

B = 7


def cocoop_rig():
    g = torch.Generator().manual_seed(9)
    case = dict(load_npz("tiny_cocoop"))
    case["image"] = torch.randn(B, 3, 32, 32, generator=g).numpy()
    case["label"] = torch.randint(0, 5, (B,), generator=g).numpy()
    return build_cocoop("tiny_cocoop", case)


def tpt_rig():
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.tpt import CustomCLIP
    from mvlpt_amd.weights import ARCHS
    arch = ARCHS["tiny"]
    torch.manual_seed(0)
    return CustomCLIP(make_cfg(arch), P.NAMES[:P.N_CLASSES], FrozenCLIP(P.state_dict(arch), device=DEV)).to(DEV)


@pytest.fixture(scope="module")
def rigs():
    model, image, label, _ = cocoop_rig()
    return {"cocoop": (model, image, label), "tpt": (tpt_rig(), None, None)}


@pytest.mark.parametrize("rig", ["cocoop", "tpt"])
def test_text_workspace_does_not_decrease_with_the_image_count(rigs, rig):
    model = rigs[rig][0]
    eng, n_cls, L = model.engine, model.prompt_learner.n_cls, model.prompt_learner.layout.shape[1]
    try:
        for segments in (1, 3):
            eng.set_text_act_ckpt(segments)
            for save in (False, True):
                figures = [eng.text_workspace_bytes(n * n_cls, L, save) for n in range(1, 17)]
                assert figures[0] > 0 and figures == sorted(figures), (segments, save, figures)
    finally:
        eng.set_text_act_ckpt(model.text_act_ckpt)


@pytest.mark.parametrize("rig", ["cocoop", "tpt"])
def test_a_budget_of_two_images_cuts_seven_into_four_chunks(rigs, rig):
    model, image, label = rigs[rig]
    n_cls, L = model.prompt_learner.n_cls, model.prompt_learner.layout.shape[1]
    budget = model.max_text_workspace_bytes
    try:
        model.max_text_workspace_bytes = model.engine.text_workspace_bytes(2 * n_cls, L, True)
        chunks = model.chunks([0] * B, [n_cls] * B, L, True)
        assert chunks == [(0, 2, 2 * n_cls), (2, 4, 2 * n_cls), (4, 6, 2 * n_cls), (6, 7, n_cls)]
        assert model.images_per_chunk(B, L, True) == 2
        if rig == "cocoop":
            assert chunks == [(0, 2, 10), (2, 4, 10), (4, 6, 10), (6, 7, 5)]
            run_cocoop(model, image, label)
            assert model.last_chunks == 4
    finally:
        model.max_text_workspace_bytes = budget
