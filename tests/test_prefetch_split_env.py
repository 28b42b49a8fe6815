"""TRAINER.MVLPT.PREFETCH_SPLIT and its environment override MVLPT_PREFETCH_SPLIT=k:c (host logic only)."""
import pytest


def test_prefetch_split_setting_and_override(monkeypatch):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import prefetch_split
    cfg = get_cfg_default()
    monkeypatch.delenv("MVLPT_PREFETCH_SPLIT", raising=False)
    assert "ViT-B/16" in cfg.TRAINER.MVLPT.PREFETCH_SPLIT_TOWERS
    cfg.MODEL.BACKBONE.NAME = "ViT-B/16"
    assert prefetch_split(cfg) == tuple(cfg.TRAINER.MVLPT.PREFETCH_SPLIT) != (0, 0)
    cfg.TRAINER.MVLPT.PREFETCH_SPLIT = (2, 128)
    assert prefetch_split(cfg) == (2, 128)
    for other in ("ViT-B/32", "ViT-L/14", "tiny"):            # not measured to pay there: one piece
        cfg.MODEL.BACKBONE.NAME = other
        assert prefetch_split(cfg) == (0, 0)
    cfg.TRAINER.MVLPT.PREFETCH_SPLIT_TOWERS = ()              # every backbone
    assert prefetch_split(cfg) == (2, 128)
    cfg.TRAINER.MVLPT.PREFETCH_SPLIT_TOWERS = ("ViT-B/16",)
    for text, want in (("0:0", (0, 0)), ("6:192", (6, 192)), (" 11 : 0 ", (11, 0))):
        monkeypatch.setenv("MVLPT_PREFETCH_SPLIT", text)
        assert prefetch_split(cfg) == want
    for bad in ("a:b", "6:", ":192", "6", "6:192:1", "-1:8"):
        monkeypatch.setenv("MVLPT_PREFETCH_SPLIT", bad)
        with pytest.raises(ValueError, match="MVLPT_PREFETCH_SPLIT.*k:c"):
            prefetch_split(cfg)
