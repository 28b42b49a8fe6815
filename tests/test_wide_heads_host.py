"""Image towers with heads wider than 64 (the ViT-H/14 family) on the host, CPU only: the architecture check of mvlpt_create, the arch
table and the state-dict inference, the config key, every trainer handing the head width to the FrozenCLIP it builds, and the
configurations that are refused before any engine exists."""
import ctypes
import dataclasses
from types import SimpleNamespace

import pytest
import torch

WIDTHS = (64, 80, 96, 112, 128)


def _create(vision_width, vision_heads, text_width=128, text_heads=2):
    from mvlpt_amd import _lib
    a = _lib.MvlptArch(48, 16, vision_width, 3, vision_heads, 77, text_width, 2, text_heads, 128, _lib.DT_F16)
    h = ctypes.c_void_p()
    rc = _lib.lib.mvlpt_create(ctypes.byref(a), ctypes.byref(h))
    msg = _lib.last_error(None)
    if rc == 0:
        _lib.lib.mvlpt_destroy(h)
    return rc, msg


@pytest.mark.parametrize("width,heads", [(640, 8), (1280, 16), (768, 8), (896, 8), (1024, 8), (128, 2)])
def test_create_accepts_the_listed_head_widths(width, heads):
    """Past the architecture check: with a device the handle exists, without one the device probe answers (there is no CPU fallback)."""
    rc, msg = _create(width, heads)
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert rc < 0 and rc != -4 and "no HIP device" in msg, (rc, msg)


@pytest.mark.parametrize("width,heads", [(576, 8), (100, 2), (704, 8), (832, 8), (1152, 8), (640, 4), (640, 0), (640, 7)])
def test_create_refuses_every_other_head_width(width, heads):
    """72, 50, 88, 104, 144, 160, no heads, a width the heads do not divide: MVLPT_ERR_UNSUPPORTED, ahead of the multiple-of-128 test."""
    rc, msg = _create(width, heads)
    assert rc == -4 and "head_dim" in msg and "80 / 96 / 112 / 128" in msg, (rc, msg)


def test_the_text_tower_stays_at_64():
    rc, msg = _create(640, 8, text_width=640, text_heads=8)
    assert rc == -4 and "head_dim" in msg


def test_arch_table():
    from mvlpt_amd.weights import ARCHS, WIDE_HEAD_ARCHS, ClipArch, get_arch
    want = {"ViT-B/32": 12, "ViT-B/16": 12, "ViT-L/14": 16, "ViT-L/14@336px": 16, "tiny": 2}
    for name, heads in want.items():
        assert ARCHS[name].vision_head_width == 64 and ARCHS[name].vision_heads == heads == ARCHS[name].vision_width // 64
    # the wide-headed backbones have a table of their own (as the ResNets have); get_arch finds them by name
    assert not set(WIDE_HEAD_ARCHS) & set(ARCHS) and all(get_arch(n) is a and a.name == n for n, a in WIDE_HEAD_ARCHS.items())
    h = WIDE_HEAD_ARCHS["ViT-H/14"]
    assert (h.vision_width, h.vision_head_width, h.vision_heads, h.vision_layers, h.embed_dim) == (1280, 80, 16, 32, 1024)
    assert (h.transformer_width, h.transformer_heads, h.transformer_layers, h.grid ** 2 + 1) == (1024, 16, 24, 257)
    t = WIDE_HEAD_ARCHS["tiny-h"]
    assert (t.vision_width, t.vision_heads, t.grid ** 2 + 1, t.embed_dim, t.transformer_width) == (640, 8, 10, 128, 128)
    # the field is the last one and defaulted; the reference's constructor arguments do not know it
    assert [f.name for f in dataclasses.fields(ClipArch)][-1] == "vision_head_width"
    assert len(h.ctor_args()) == 10 and h.ctor_args() == dataclasses.replace(h, vision_head_width=64).ctor_args()


def test_random_weights_and_state_dict_inference():
    from mvlpt_amd.weights import WIDE_HEAD_ARCHS, arch_from_state_dict, make_state_dict
    arch = WIDE_HEAD_ARCHS["tiny-h"]
    sd = make_state_dict(arch, 3)
    assert sd["visual.transformer.resblocks.2.attn.in_proj_weight"].shape == (1920, 640) and sd["visual.proj"].shape == (640, 128)
    assert arch_from_state_dict(sd).vision_heads == 10            # what the reference's build_model would say: the caller has to know
    got = arch_from_state_dict(sd, "tiny-h", vision_head_width=80)
    assert got == arch and got.vision_heads == 8
    assert arch_from_state_dict(sd, vision_head_width=128).vision_heads == 5
    for bad in (96, 112, 0, -80):
        with pytest.raises(ValueError, match="not a multiple of the head width"):
            arch_from_state_dict(sd, vision_head_width=bad)


def _cfg(name="tiny-h", width=None):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = name
    cfg.INPUT.SIZE = (48, 48)
    cfg.TRAINER.MVLPT.COOP.N_CTX = 4
    cfg.TRAINER.MVLPT.VPT.N_CTX = 0
    if width is not None:
        cfg.MODEL.BACKBONE.VISION_HEAD_WIDTH = width
    return cfg


def test_config_key():
    from mvlpt_amd.config import get_cfg_default, read_vision_head_width
    cfg = get_cfg_default()
    assert cfg.MODEL.BACKBONE.VISION_HEAD_WIDTH == 0
    for name in ("ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px", "tiny", "RN50", "tiny-rn", "a name of no table"):
        cfg.MODEL.BACKBONE.NAME = name
        assert read_vision_head_width(cfg) == 64, name
    for name in ("ViT-H/14", "tiny-h"):
        cfg.MODEL.BACKBONE.NAME = name
        assert read_vision_head_width(cfg) == 80
    for w in WIDTHS:
        cfg.merge_from_list(["MODEL.BACKBONE.VISION_HEAD_WIDTH", str(w)])
        assert read_vision_head_width(cfg) == w
    for bad in (72, 88, 104, 32, 256, -80, 80.0, "80", True):
        cfg.MODEL.BACKBONE.VISION_HEAD_WIDTH = bad
        with pytest.raises(ValueError, match="64, 80, 96, 112, 128"):
            read_vision_head_width(cfg)
    del cfg.MODEL.BACKBONE["VISION_HEAD_WIDTH"]          # a config tree from before the key
    cfg.MODEL.BACKBONE.NAME = "ViT-B/16"
    assert read_vision_head_width(cfg) == 64


class _Stop(Exception):
    pass


def _recorder(seen):
    def ctor(*a, **k):
        seen.append(k.get("vision_head_width"))
        raise _Stop()
    return ctor


def _self(cfg):
    return SimpleNamespace(cfg=cfg, dm=SimpleNamespace(dataset=SimpleNamespace(classnames=["a", "b"]), lab2cname={0: "a", 1: "b"}),
                           _sd_arg={}, device="cpu", single_template=True)


def _patched(monkeypatch, seen):
    import mvlpt_amd.cocoop as co
    import mvlpt_amd.trainer as tr
    import mvlpt_amd.zsclip as zs
    for mod in (tr, co, zs):
        monkeypatch.setattr(mod, "FrozenCLIP", _recorder(seen))
    return tr, co, zs


@pytest.mark.parametrize("name,width,want", [("tiny-h", None, 80), ("tiny", None, 64), ("tiny", 80, 80), ("ViT-H/14", 0, 80), ("tiny-h", 128, 128)])
def test_every_trainer_that_runs_hands_the_head_width_to_its_frozen_clip(monkeypatch, name, width, want):
    """CoOp (MVLPT with VPT.N_CTX 0), MVLPT-CoCoOp without visual prompts, CoCoOp and the two zero-shot trainers reach FrozenCLIP with
    vision_head_width = the key (0: the named backbone's own)."""
    seen = []
    tr, co, zs = _patched(monkeypatch, seen)
    cocoop_route = _cfg(name, width)
    cocoop_route.TRAINER.MVLPT.COOP.N_CTX, cocoop_route.TRAINER.MVLPT.COCOOP.N_CTX = 0, 4
    builds = [(tr.MVLPT.build_model, _cfg(name, width)), (tr.MVLPT.build_model, cocoop_route), (co.CoCoOp.build_model, _cfg(name, width)),
              (zs.ZeroshotCLIP.build_model, _cfg(name, width)), (zs.ZeroshotCLIP2.build_model, _cfg(name, width))]
    for build, cfg in builds:
        with pytest.raises(_Stop):
            build(_self(cfg))
    assert seen == [want] * len(builds)


def _refused():
    def vpt(cfg):
        cfg.TRAINER.MVLPT.VPT.N_CTX, cfg.TRAINER.MVLPT.COOP.N_CTX = 4, 0

    def upt(cfg):
        cfg.TRAINER.MVLPT.VPT.N_CTX, cfg.TRAINER.MVLPT.COOP.N_CTX = 4, 4

    def cocoop_vpt(cfg):
        cfg.TRAINER.MVLPT.VPT.N_CTX, cfg.TRAINER.MVLPT.COOP.N_CTX, cfg.TRAINER.MVLPT.COCOOP.N_CTX = 4, 0, 4

    def fp32(cfg):
        cfg.TRAINER.MVLPT.PREC = "fp32"

    return [("vpt", vpt, "visual prompts"), ("upt", upt, "visual prompts"), ("mvlpt-cocoop + vpt", cocoop_vpt, "visual prompts"),
            ("prec fp32", fp32, "operand pairs")]


@pytest.mark.parametrize("what,change,message", _refused(), ids=[r[0] for r in _refused()])
@pytest.mark.parametrize("name,width", [("tiny-h", None), ("ViT-H/14", None), ("tiny", 96)])
def test_refused_configurations_stop_before_any_engine(monkeypatch, name, width, what, change, message):
    seen = []
    tr, _co, _zs = _patched(monkeypatch, seen)
    cfg = _cfg(name, width)
    change(cfg)
    with pytest.raises(ValueError, match=message) as e:
        tr.MVLPT.build_model(_self(cfg))
    assert "frozen, prompt-free and forward-only" in str(e.value) and seen == []
    # the same configuration on heads of 64 is none of this check's business
    cfg = _cfg("tiny", None)
    change(cfg)
    with pytest.raises(_Stop):
        tr.MVLPT.build_model(_self(cfg))
    assert seen == [64]


def test_cocoop_with_fp32_operands_is_refused_as_well(monkeypatch):
    seen = []
    _tr, co, _zs = _patched(monkeypatch, seen)
    cfg = _cfg()
    cfg.TRAINER.COCOOP.PREC = "fp32"
    with pytest.raises(ValueError, match="operand pairs"):
        co.CoCoOp.build_model(_self(cfg))
    assert seen == []


def test_frozen_clip_builds_its_arch_with_the_head_width(monkeypatch):
    """FrozenCLIP(sd, vision_head_width=80) describes a tiny-h state dict as 8 heads of 80 to its engine; the linear probe's
    extract_features runs whatever FrozenCLIP it is given."""
    import mvlpt_amd.model as M
    from mvlpt_amd.weights import WIDE_HEAD_ARCHS, make_state_dict
    from tests.fake_engine import OracleEngine

    class _Engine(OracleEngine):
        device = torch.device("cpu")

        def set_precision(self, mode):
            self.precision = mode

        @classmethod
        def from_state_dict(cls, sd, compute_dtype="fp16", device=None, arch=None, activation="quick_gelu"):
            return cls(sd, arch)

    monkeypatch.setattr(M, "Engine", _Engine)
    sd = make_state_dict(WIDE_HEAD_ARCHS["tiny-h"], 3)
    clip = M.FrozenCLIP(sd, vision_head_width=80)
    assert clip.arch.vision_heads == 8 and clip.engine.arch.vision_heads == 8
    assert M.FrozenCLIP(sd).arch.vision_heads == 10
    from mvlpt_amd.linear_probe import extract_features
    image = torch.randn(2, 3, 48, 48, generator=torch.Generator().manual_seed(0))
    feats, labels = extract_features(clip, [(image, torch.tensor([1, 0]))])
    assert feats.shape == (2, 128) and labels.tolist() == [1, 0]
    # eight heads of 80, not ten of 64: the two descriptions of the same weights give different features
    other, _ = extract_features(M.FrozenCLIP(sd), [(image, torch.tensor([1, 0]))])
    assert float(abs(torch.as_tensor(feats) - torch.as_tensor(other)).max()) > 1e-3


def test_header_declares_the_wide_entry_and_lib_binds_it():
    import os
    import re
    from mvlpt_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mvlpt_hip.h")).read()
    m = re.search(r"\bint\s+mvlpt_op_attention_wide_fwd\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m and len(_lib.SIGNATURES["mvlpt_op_attention_wide_fwd"][1]) == m.group(1).count(",") + 1 == 10
    assert hasattr(_lib.lib, "mvlpt_op_attention_wide_fwd")
