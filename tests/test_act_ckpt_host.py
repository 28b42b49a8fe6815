"""TRAINER.ACT_CKPT on the host (no GPU): the segment plan against torch's own checkpoint_sequential, and the way from the config
key to the engine for the three model classes, on the oracle-backed stand-in engine."""
import pytest
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint_sequential

from tests.fake_engine import OracleEngine, OracleFrozenCLIP


# ------------------------------------------------------------------------------------------------ the plan
class _Counting(nn.Module):
    def __init__(self, index, log):
        super().__init__()
        self.index, self.log = index, log

    def forward(self, x):
        self.log.append(self.index)
        return x * 1.5 + 1.0


def _torch_plan(layers, segments):
    """[(first, last_exclusive, checkpointed)] as torch itself cuts `layers` modules: the modules its first backward runs again
    are the checkpointed ones, and they come back segment by segment, from the last checkpointed segment to the first."""
    log = []
    blocks = nn.Sequential(*[_Counting(i, log) for i in range(layers)])
    x = torch.ones(2, requires_grad=True)
    y = checkpoint_sequential(blocks, segments, x, use_reentrant=True)
    assert log == list(range(layers))
    del log[:]
    y.sum().backward()
    runs = []                                  # maximal ascending runs of the recomputation = the checkpointed segments
    for i in log:
        if runs and i == runs[-1][-1] + 1:
            runs[-1].append(i)
        else:
            runs.append([i])
    assert runs == sorted(runs, reverse=True), "torch recomputes the segments from the back"
    plan = [(r[0], r[-1] + 1, True) for r in reversed(runs)]
    first_saved = plan[-1][1] if plan else 0
    assert sorted(log) == list(range(first_saved)), "the checkpointed modules are the leading ones"
    return plan + [(first_saved, layers, False)]


@pytest.mark.parametrize("layers", [2, 5, 12])
def test_plan_is_torchs_checkpoint_sequential(layers):
    from mvlpt_amd.model import checkpoint_segments
    for n in range(1, layers + 4):
        # torch takes at most one segment per module (more: its segment size is 0 and it raises); the engine clamps there
        want = _torch_plan(layers, min(n, layers))
        got = checkpoint_segments(layers, n)
        assert got == want, f"layers={layers} n={n}"
        assert got[0][0] == 0 and got[-1][1] == layers and all(a[1] == b[0] for a, b in zip(got, got[1:]))


def test_plan_examples_and_largest_segment_is_not_monotonic():
    from mvlpt_amd.model import checkpoint_segments
    sizes = lambda k: [b - a for a, b, _ in checkpoint_segments(12, k)]
    assert sizes(5) == [2, 2, 2, 2, 4] and sizes(7) == [1] * 6 + [6] and sizes(1) == [12] and sizes(40) == [1] * 12
    assert max(sizes(7)) > max(sizes(5))
    assert checkpoint_segments(12, 0) == checkpoint_segments(12, 1) == [(0, 12, False)]


# ------------------------------------------------------------------------------------------------ config -> engine
class _RecordingEngine(OracleEngine):
    precision = 0                       # MVLPT_PREC_FAST: the CoCoOp models leave an explicit mode alone

    def __init__(self, sd, arch):
        super().__init__(sd, arch)
        self.act_ckpt_calls = []

    def set_text_act_ckpt(self, n):
        self.act_ckpt_calls.append(n)


def _clip():
    from mvlpt_amd.weights import ARCHS, make_state_dict
    arch = ARCHS["tiny"]
    sd = make_state_dict(arch, 1)
    clip = OracleFrozenCLIP(sd, arch)
    clip.engine = _RecordingEngine(sd, arch)
    return clip


def _cfg(route, act_ckpt):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    if route == "model":
        cfg.TRAINER.MVLPT.COOP.N_CTX = 4
    elif route == "cocoop":
        cfg.TRAINER.COCOOP.N_CTX = 4
    else:
        cfg.TRAINER.MVLPT.COCOOP.N_CTX = 4
    if act_ckpt is None:
        del cfg.TRAINER["ACT_CKPT"]
    else:
        cfg.TRAINER.ACT_CKPT = act_ckpt
    return cfg


def _build(route, cfg, clip):
    names = ["dog", "sea horse", "cat"]
    if route == "model":
        from mvlpt_amd.model import CustomCLIP
    elif route == "cocoop":
        from mvlpt_amd.cocoop import CustomCLIP
    else:
        from mvlpt_amd.mvlpt_cocoop import CustomCLIP
    return CustomCLIP(cfg, names, clip)


@pytest.mark.parametrize("route", ["model", "cocoop", "mvlpt_cocoop"])
def test_config_key_reaches_the_engine(route):
    clip = _clip()
    model = _build(route, _cfg(route, 3), clip)
    assert clip.engine.act_ckpt_calls == [3] and model.text_act_ckpt == 3
    clip = _clip()
    model = _build(route, _cfg(route, None), clip)
    assert clip.engine.act_ckpt_calls == [1] and model.text_act_ckpt == 1, "a config without the key is ACT_CKPT = 1"


def test_an_engine_without_the_setting_refuses_more_than_one_segment():
    """The stand-in engine of the other host tests has no checkpointing: ACT_CKPT = 1 is what it does, anything else is an error."""
    from mvlpt_amd.weights import ARCHS, make_state_dict
    arch = ARCHS["tiny"]
    sd = make_state_dict(arch, 1)
    assert _build("model", _cfg("model", 1), OracleFrozenCLIP(sd, arch)).text_act_ckpt == 1
    with pytest.raises(ValueError, match="ACT_CKPT"):
        _build("model", _cfg("model", 2), OracleFrozenCLIP(sd, arch))
