"""CPU checks of the host side of test-time prompt tuning (mvlpt_amd.tpt, mvlpt_amd.transforms.ViewTransform): k from the config,
every refusal with the key it names, the descriptor layout of the views, the trainer's registration.  No GPU."""
import os
import sys

import pytest
import torch

from mvlpt_amd.config import get_cfg_default

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_keys_and_k():
    from mvlpt_amd.tpt import tpt_settings
    cfg = get_cfg_default()
    assert cfg.TRAINER.TPT == {"N_VIEWS": 64, "SELECTION_P": 0.1, "STEPS": 1, "LR": 5e-3, "N_CTX": 4, "CTX_INIT": "a photo of a",
                               "PREC": "fp16"}
    assert tpt_settings(cfg) == (64, 6, 1, 5e-3)                  # k = max(1, int(64 * 0.1))
    for v, p, k in [(8, 0.25, 2), (8, 0.1, 1), (1, 1.0, 1), (128, 0.1, 12), (64, 1.0, 64), (7, 0.5, 3)]:
        cfg.TRAINER.TPT.N_VIEWS, cfg.TRAINER.TPT.SELECTION_P = v, p
        assert tpt_settings(cfg)[:2] == (v, k)
    cfg.merge_from_list(["TRAINER.TPT.N_VIEWS", "32", "TRAINER.TPT.SELECTION_P", "0.5", "TRAINER.TPT.STEPS", "2"])
    assert tpt_settings(cfg) == (32, 16, 2, 5e-3)


@pytest.mark.parametrize("key,value,named", [
    ("TRAINER.MVLPT.COOP.CSC", True, "COOP.CSC"),
    ("TRAINER.TPT.N_VIEWS", 0, "TPT.N_VIEWS"), ("TRAINER.TPT.N_VIEWS", 129, "TPT.N_VIEWS"), ("TRAINER.TPT.N_VIEWS", -3, "TPT.N_VIEWS"),
    ("TRAINER.TPT.SELECTION_P", 0.0, "TPT.SELECTION_P"), ("TRAINER.TPT.SELECTION_P", 1.5, "TPT.SELECTION_P"),
    ("TRAINER.TPT.SELECTION_P", -0.1, "TPT.SELECTION_P"), ("TRAINER.TPT.SELECTION_P", float("nan"), "TPT.SELECTION_P"),
    ("TRAINER.MVLPT.VPT.N_CTX", 4, "VPT.N_CTX"),
    ("TRAINER.MVLPT.COCOOP.N_CTX", 4, "COCOOP.N_CTX"), ("TRAINER.MVLPT.COOP.N_DEEP", 1, "COOP.N_DEEP"),
    ("TRAINER.TPT.STEPS", -1, "TPT.STEPS"), ("TRAINER.TPT.PREC", "fp8", "TPT.PREC"),
])
def test_refusals_name_their_key(key, value, named):
    from mvlpt_amd.tpt import tpt_settings
    cfg = get_cfg_default()
    node = cfg
    parts = key.split(".")
    for p in parts[:-1]:
        node = node[p]
    node[parts[-1]] = value
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        tpt_settings(cfg)


def test_class_sharding_over_several_ranks_is_refused():
    from mvlpt_amd.tpt import CustomCLIP, tpt_settings
    cfg = get_cfg_default()
    assert tpt_settings(cfg, world_size=1)[0] == 64
    with pytest.raises(ValueError, match="class sharding over 2 ranks"):
        tpt_settings(cfg, world_size=2)
    model = object.__new__(CustomCLIP)
    CustomCLIP.enable_class_sharding(model, 0, 1)                # one rank: nothing is sharded
    with pytest.raises(ValueError, match="class sharding over 2 ranks"):
        CustomCLIP.enable_class_sharding(model, 0, 2)


def test_prompt_cfg_takes_coop_when_it_asks_for_a_context():
    from mvlpt_amd.tpt import prompt_cfg
    cfg = get_cfg_default()
    c = prompt_cfg(cfg).TRAINER.MVLPT.COOP
    assert (c.N_CTX, c.CTX_INIT, c.CLASS_TOKEN_POSITION) == (4, "a photo of a", "end")
    assert cfg.TRAINER.MVLPT.COOP.N_CTX == 0                     # the caller's config is not touched
    cfg.TRAINER.MVLPT.COOP.N_CTX, cfg.TRAINER.MVLPT.COOP.CTX_INIT = 16, ""
    c = prompt_cfg(cfg).TRAINER.MVLPT.COOP
    assert (c.N_CTX, c.CTX_INIT, c.CLASS_TOKEN_POSITION) == (16, "", "middle")
    cfg = get_cfg_default()
    cfg.TRAINER.TPT.N_CTX, cfg.TRAINER.TPT.CTX_INIT = 0, ""
    with pytest.raises(ValueError, match="TPT.N_CTX"):
        prompt_cfg(cfg)


def test_prompt_learner_has_coop_state_dict_keys_and_ctx_init():
    from mvlpt_amd.model import MultitaskVLPromptLearner
    from mvlpt_amd.tpt import prompt_cfg
    from mvlpt_amd.weights import ARCHS, make_state_dict
    from tests.fake_engine import OracleFrozenCLIP
    arch = ARCHS["tiny"]
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (arch.image_resolution,) * 2
    clip = OracleFrozenCLIP(make_state_dict(arch, seed=2), arch)
    pl = MultitaskVLPromptLearner(prompt_cfg(cfg), ["cat", "red fox"], clip)
    assert sorted(pl.state_dict()) == ["ctx", "token_prefix", "token_suffix"] and pl.ctx.shape == (4, arch.transformer_width)
    ids = clip.tokenizer.tokenize("a photo of a")
    assert torch.equal(pl.ctx.detach(), clip.token_embedding(ids)[0, 1:5].float())
    cfg.TRAINER.MVLPT.COOP.N_CTX = 4                             # a CoOp configuration: the same keys
    coop = MultitaskVLPromptLearner(cfg, ["cat", "red fox"], clip)
    assert sorted(coop.state_dict()) == sorted(pl.state_dict())


# ------------------------------------------------------------------------------------------------ views
def _transforms(seed, transforms=None):
    from mvlpt_amd.transforms import DeviceTransform
    g = torch.Generator().manual_seed(seed)
    return (DeviceTransform(None, size=32, train=False), DeviceTransform(None, size=32, train=True, generator=g, transforms=transforms))


def _fields(d):
    return tuple(getattr(d, n) for n, _ in type(d)._fields_ if n != "offset")


@pytest.mark.parametrize("transforms", [None, ["random_crop", "random_flip", "colorjitter", "cutout", "normalize"]],
                         ids=["default", "augmented"])
def test_view_descriptors_layout_offsets_and_draw_order(transforms):
    from mvlpt_amd.transforms import ViewTransform
    V, shapes, offsets = 5, [(40, 60), (33, 21), (64, 64)], [7000, 0, 123456789012]
    vt = ViewTransform(*_transforms(3, transforms), V)
    descs, augs = vt.describe_views(shapes, offsets)
    assert len(descs) == len(shapes) * V and (augs is None) == (transforms is None)
    test_t, train_t = _transforms(3, transforms)          # the same generator state, driven by hand
    for g, (shape, off) in enumerate(zip(shapes, offsets)):
        want0 = test_t.describe([shape])[0][0]
        wt, wa, _ = train_t.describe_aug([shape] * (V - 1))          # image-major: image g's V - 1 draws come before image g + 1's
        assert all(descs[g * V + j].offset == off for j in range(V))                       # one image in the source, V descriptors
        assert _fields(descs[g * V]) == _fields(want0) and descs[g * V].flip == 0          # view 0: Resize + CenterCrop
        assert (descs[g * V].height, descs[g * V].width) == shape
        for j in range(V - 1):
            assert _fields(descs[g * V + 1 + j]) == _fields(wt[j])
            if augs is not None:
                assert bytes(augs[g * V + 1 + j]) == bytes(wa[j])
        if augs is not None:
            assert bytes(augs[g * V]) == bytes(type(augs[0])())                            # view 0: the empty augmentation
    # the train views differ from one another and from the test view
    assert len({_fields(descs[j]) for j in range(V)}) > 2


def test_view_transform_refusals():
    from mvlpt_amd.transforms import DeviceTransform, ViewTransform
    test_t, train_t = _transforms(0)
    with pytest.raises(ValueError, match="train=False"):
        ViewTransform(train_t, train_t, 4)
    with pytest.raises(ValueError, match="n_views"):
        ViewTransform(test_t, train_t, 0)
    with pytest.raises(ValueError, match="normalize"):
        ViewTransform(test_t, DeviceTransform(None, size=32, train=True, transforms=["random_resized_crop"]), 4)
    vt = ViewTransform(test_t, train_t, 1)                       # one view: the test view alone, nothing is drawn
    state = train_t.generator.get_state()
    descs, _ = vt.describe_views([(40, 60)], [0])
    assert len(descs) == 1 and torch.equal(train_t.generator.get_state(), state)


def test_loaders_serve_views_only_on_request():
    from mvlpt_amd.data import Datum, DeviceLoader
    cfg = get_cfg_default()
    items = [Datum(impath=f"{i}.jpg", label=i % 2, domain=0, classname=str(i % 2)) for i in range(4)]
    test_loader, train_loader = DeviceLoader(cfg, items, train=False), DeviceLoader(cfg, items, train=True)
    assert test_loader.n_views == 0 and train_loader.n_views == 0
    test_loader.request_views(8)
    assert test_loader.n_views == 8 and test_loader.transform is None          # unbound: the transform is built at bind time
    with pytest.raises(ValueError, match="evaluation loaders"):
        train_loader.request_views(8)


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_is_registered_and_evaluation_only():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train as launcher
    finally:
        sys.path.pop(0)
    from mvlpt_amd.tpt import TPT
    from mvlpt_amd.trainer import MVLPT
    assert "TPT" in launcher.TRAINERS and "TPT" in launcher.EVAL_ONLY_TRAINERS
    assert launcher.trainer_class("TPT") is TPT and issubclass(TPT, MVLPT) and TPT.test is MVLPT.test
    assert [launcher.trainer_class(n).__name__ for n in launcher.TRAINERS] == list(launcher.TRAINERS)
    with pytest.raises(RuntimeError, match="nothing to train"):
        TPT.forward_backward(object.__new__(TPT), {"img": None})


# ------------------------------------------------------------------------------------------------ C entries: refused before any HIP call
P_ = 4096      # a non-null, 16-byte aligned "pointer": never dereferenced, the refusal comes first


@pytest.mark.parametrize("call,text", [
    (lambda L, C: L.lib.mvlpt_tpt_workspace_bytes(1, 129, 10, 64, 1, C.byref(C.c_int64())),
     "tpt_workspace_bytes: V must lie in [1, MVLPT_TPT_MAX_VIEWS]"),
    (lambda L, C: L.lib.mvlpt_tpt_workspace_bytes(1, 8, 10, 1028, 1, C.byref(C.c_int64())),
     "tpt_workspace_bytes: e must be a multiple of 4 in [4, 1024]"),
    (lambda L, C: L.lib.mvlpt_tpt_workspace_bytes(1, 8, 10, 64, 9, C.byref(C.c_int64())), "tpt_workspace_bytes: k must lie in [1, V]"),
    (lambda L, C: L.lib.mvlpt_tpt_workspace_bytes(1, 8, 0, 64, 1, C.byref(C.c_int64())),
     "tpt_workspace_bytes: C must lie in [1, MVLPT_TPT_MAX_CLASSES]"),
    (lambda L, C: L.lib.mvlpt_tpt_workspace_bytes(1, 8, 10, 64, 1, None), "tpt_workspace_bytes: null argument"),
    (lambda L, C: L.lib.mvlpt_op_tpt_head_fwd(None, P_, 100.0, 1, 8, 10, 64, 1, P_, P_, P_, None, P_, 1 << 30, None),
     "op_tpt_head_fwd: null argument"),
    (lambda L, C: L.lib.mvlpt_op_tpt_head_fwd(P_, P_, 100.0, 1, 8, 10, 64, 1, P_, P_, P_, None, P_, 16, None),
     "op_tpt_head_fwd: the workspace is smaller than mvlpt_tpt_workspace_bytes"),
    (lambda L, C: L.lib.mvlpt_op_tpt_head_fwd(P_ + 4, P_, 100.0, 1, 8, 10, 64, 1, P_, P_, P_, None, P_, 1 << 30, None),
     "op_tpt_head_fwd: img and txt must be 16-byte aligned"),
    (lambda L, C: L.lib.mvlpt_op_tpt_head_bwd(None, 100.0, 1, 8, 10, 64, 0, P_, P_, 1 << 30, None), "op_tpt_head_bwd: k must lie in [1, V]"),
    (lambda L, C: L.lib.mvlpt_op_tpt_head_bwd(None, 100.0, 1, 8, 10, 64, 1, P_, None, 1 << 30, None),
     "op_tpt_head_bwd: the workspace is smaller than mvlpt_tpt_workspace_bytes"),
])
def test_c_entries_refuse_before_any_launch(call, text):
    import ctypes as C
    from mvlpt_amd import _lib as L
    assert call(L, C) == L.ERR_ARG
    assert L.last_error(None).startswith(text), L.last_error(None)


def test_workspace_bytes_is_a_function_of_the_sizes():
    import ctypes as C
    from mvlpt_amd import _lib as L
    out = C.c_int64()
    assert L.lib.mvlpt_tpt_workspace_bytes(16, 64, 1000, 512, 6, C.byref(out)) == 0
    # normalised rows of both operands dominate: G (V + C) e floats; the selected views' logp and dz add 2 G k C
    floats = 16 * (64 + 1000) * 512 + 2 * 16 * 6 * 1000
    assert floats * 4 <= out.value <= floats * 4 * 1.02
