"""MODEL.BACKBONE.ACTIVATION on the host, CPU only: the config key and its refusal, every trainer handing the value to the engine it
builds, and the C ABI's new symbols declared in the header and bound under the same names."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mvlpt_set_activation", "mvlpt_get_activation", "mvlpt_op_activation_fwd", "mvlpt_op_activation_bwd"]


def _cfg(activation=None):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    if activation is not None:
        cfg.MODEL.BACKBONE.ACTIVATION = activation
    return cfg


def test_config_key_default_override_and_refusal():
    from mvlpt_amd.config import get_cfg_default, read_activation
    cfg = get_cfg_default()
    assert cfg.MODEL.BACKBONE.ACTIVATION == "quick_gelu" and read_activation(cfg) == "quick_gelu"
    cfg.merge_from_list(["MODEL.BACKBONE.ACTIVATION", "gelu"])
    assert read_activation(cfg) == "gelu"
    for bad in ("GELU", "relu", "", "quickgelu", 1):
        cfg.MODEL.BACKBONE.ACTIVATION = bad
        with pytest.raises(ValueError, match="'quick_gelu' and 'gelu'"):
            read_activation(cfg)
    del cfg.MODEL.BACKBONE["ACTIVATION"]          # a config tree from before the key
    assert read_activation(cfg) == "quick_gelu"


class _Stop(Exception):
    pass


def _recorder(seen):
    def ctor(*a, **k):
        seen.append(k.get("activation"))
        raise _Stop()
    return ctor


def _self(cfg):
    return SimpleNamespace(cfg=cfg, dm=SimpleNamespace(dataset=SimpleNamespace(classnames=["a", "b"]), lab2cname={0: "a", 1: "b"}),
                           _sd_arg={}, device="cpu", single_template=True)


@pytest.mark.parametrize("activation", [None, "quick_gelu", "gelu"])
def test_every_trainer_hands_the_key_to_its_frozen_clip(monkeypatch, activation):
    """MVLPT (CoOp / VPT / UPT), its CoCoOp route, CoCoOp and the two zero-shot trainers: build_model passes activation = the key."""
    import mvlpt_amd.cocoop as co
    import mvlpt_amd.trainer as tr
    import mvlpt_amd.zsclip as zs
    seen = []
    for mod in (tr, co, zs):
        monkeypatch.setattr(mod, "FrozenCLIP", _recorder(seen))
    want = activation or "quick_gelu"
    builds = []
    for cocoop_n_ctx in (0, 4):
        cfg = _cfg(activation)
        cfg.TRAINER.MVLPT.COOP.N_CTX, cfg.TRAINER.MVLPT.COCOOP.N_CTX = (0 if cocoop_n_ctx else 4), cocoop_n_ctx
        builds.append((tr.MVLPT.build_model, cfg))
    builds += [(co.CoCoOp.build_model, _cfg(activation)), (zs.ZeroshotCLIP.build_model, _cfg(activation)),
               (zs.ZeroshotCLIP2.build_model, _cfg(activation))]
    for build, cfg in builds:
        with pytest.raises(_Stop):
            build(_self(cfg))
    assert seen == [want] * len(builds)


@pytest.mark.parametrize("build", ["mvlpt", "cocoop", "zsclip"])
def test_a_bad_key_stops_the_build_with_the_two_accepted_values(monkeypatch, build):
    import mvlpt_amd.cocoop as co
    import mvlpt_amd.trainer as tr
    import mvlpt_amd.zsclip as zs
    for mod in (tr, co, zs):
        monkeypatch.setattr(mod, "FrozenCLIP", _recorder([]))
    fn = {"mvlpt": tr.MVLPT.build_model, "cocoop": co.CoCoOp.build_model, "zsclip": zs.ZeroshotCLIP.build_model}[build]
    cfg = _cfg("swish")
    cfg.TRAINER.MVLPT.COOP.N_CTX = 4
    with pytest.raises(ValueError, match="'quick_gelu' and 'gelu'"):
        fn(_self(cfg))


def test_frozen_clip_hands_the_activation_to_its_engine(monkeypatch):
    """FrozenCLIP(activation=...) -> Engine.from_state_dict(..., activation): what the trainers' engines and the linear probe's
    extract_features (which runs whatever FrozenCLIP it is given) end up with."""
    import mvlpt_amd.model as M
    from mvlpt_amd.weights import ARCHS
    from tests.golden_util import tiny_state_dict

    class _Engine(OracleEngine):
        device = torch.device("cpu")

        def set_precision(self, mode):
            self.precision = mode

        @classmethod
        def from_state_dict(cls, sd, compute_dtype="fp16", device=None, arch=None, activation="quick_gelu"):
            eng = cls(sd, arch)
            eng.activation = activation
            return eng

    monkeypatch.setattr(M, "Engine", _Engine)
    sd = tiny_state_dict()
    assert M.FrozenCLIP(sd, arch=ARCHS["tiny"]).engine.activation == "quick_gelu"
    clip = M.FrozenCLIP(sd, arch=ARCHS["tiny"], activation="gelu")
    assert clip.engine.activation == "gelu"
    from mvlpt_amd.linear_probe import extract_features
    image = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    feats, labels = extract_features(clip, [(image, torch.tensor([1, 0]))])
    assert feats.shape == (2, ARCHS["tiny"].embed_dim) and labels.tolist() == [1, 0]


def test_engine_refuses_an_unknown_activation_before_it_touches_a_device():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    with pytest.raises(ValueError, match="'quick_gelu' and 'gelu'"):
        Engine(ARCHS["tiny"], activation="relu")


def test_header_declares_the_new_symbols_and_lib_binds_them():
    from mvlpt_amd import _lib
    header = open(os.path.join(ROOT, "include", "mvlpt_hip.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/mvlpt_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in mvlpt_amd/_lib.py"
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, f"{name}: argument count differs from the header"
        assert hasattr(_lib.lib, name)
    enums = dict(re.findall(r"\b(MVLPT_ACT_\w+)\s*=\s*(-?\d+)", header))
    assert enums == {"MVLPT_ACT_QUICKGELU": "0", "MVLPT_ACT_GELU": "1", "MVLPT_ACT_OUT_SINGLE": "0", "MVLPT_ACT_OUT_PAIR": "1",
                     "MVLPT_ACT_OUT_MIXED": "2"}
    assert (_lib.ACT_QUICKGELU, _lib.ACT_GELU) == (0, 1) and (_lib.ACT_OUT_SINGLE, _lib.ACT_OUT_PAIR, _lib.ACT_OUT_MIXED) == (0, 1, 2)
    from mvlpt_amd import engine as E
    assert callable(E.Engine.set_activation) and callable(E.Engine.op_activation_fwd) and callable(E.Engine.op_activation_bwd)
