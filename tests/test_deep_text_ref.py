"""CPU checks of tests/deep_text_ref.py, the restatement the GPU tests of deep language prompting are held to.

Its hand-written backward (dctx, dctx_deep) and its features are compared with torch autograd in float64 over the same oracle
functions; n_deep = 0 must be oracle.clip_oracle's own text encoder; and two wrong restatements (one that forgets to zero the
overwritten rows' gradient, one that adds the positional embedding to the replaced rows) must lie more than 10 x the project's 1e-3
bar away, which shows that a comparison at that bar can see either mistake."""
import contextlib

import pytest
import torch

from oracle import clip_oracle as O
from tests import deep_text_ref as R

BAR = 1e-3               # the project's bar (tests/test_hip_model.py), normalised by max|ref|
EXACT = 1e-9             # float64 autograd against the float64 hand-written backward: rounding only
CUT_L = 11               # CUT_CONTEXTLEN: the longest prompt of NAME_LENS (SOT + 4 ctx + 4 name tokens + '.' + EOT)


def rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


@contextlib.contextmanager
def float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@pytest.fixture(scope="module")
def sd():
    from mvlpt_amd.weights import make_state_dict
    return make_state_dict(R.deep_arch(), seed=11)


def _double(d):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


@pytest.mark.parametrize("position", ["end", "middle"])
@pytest.mark.parametrize("n_deep", [1, 2, 3])
@pytest.mark.parametrize("L", [77, CUT_L])
def test_hand_backward_equals_autograd_in_float64(sd, n_deep, position, L):
    with float64():
        sd64 = _double(sd)
        I = _double(R.text_inputs(L, position, n_deep))
        ctx = I["ctx"].clone().requires_grad_(True)
        deep = I["ctx_deep"].clone().requires_grad_(True)
        feat_ag, _ = R.text_fwd_deep(sd64, ctx, deep, I["prefix"], I["suffix"], I["layout"], I["eot"], heads=R.TEXT_HEADS)
        (feat_ag * I["dfeat"]).sum().backward()
        with torch.no_grad():
            feat, tctx = R.text_fwd_deep(sd64, I["ctx"], I["ctx_deep"], I["prefix"], I["suffix"], I["layout"], I["eot"], heads=R.TEXT_HEADS)
            dctx, ddeep = R.text_bwd_deep(sd64, I["dfeat"], tctx)
        e = {"features": rel(feat, feat_ag.detach()), "dctx": rel(dctx, ctx.grad), "dctx_deep": rel(ddeep, deep.grad)}
        print(f"n_deep {n_deep} {position} L {L}: {e}")
        assert max(e.values()) < EXACT, e
        assert float(ddeep.abs().max()) > 0 and float(dctx.abs().max()) > 0

        # the two wrong restatements are far outside the bar
        with torch.no_grad():
            dctx_nz, ddeep_nz = R.text_bwd_deep(sd64, I["dfeat"], tctx, forget_zeroing=True)
            feat_pos, _ = R.text_fwd_deep(sd64, I["ctx"], I["ctx_deep"], I["prefix"], I["suffix"], I["layout"], I["eot"],
                                          heads=R.TEXT_HEADS, need_bwd=False, add_pos=True)
        w = {"no zeroing, dctx": rel(dctx_nz, dctx), "added pos, features": rel(feat_pos, feat)}
        print(f"   wrong variants: {w}")
        assert w["no zeroing, dctx"] > 10 * BAR, w
        assert w["added pos, features"] > 10 * BAR, w
        if n_deep > 1:      # the gradient that leaks through layer l's overwrite also reaches the deep rows of the layers in front
            leak = rel(ddeep_nz[:-1], ddeep[:-1])
            print(f"   no zeroing, dctx_deep[:-1]: {leak:.3e}")
            assert leak > 10 * BAR


@pytest.mark.parametrize("position", ["end", "middle"])
def test_no_deep_prompts_is_the_oracles_text_encoder(sd, position):
    I = R.text_inputs(77, position, 0)
    with torch.no_grad():
        feat, tctx = R.text_fwd_deep(sd, I["ctx"], None, I["prefix"], I["suffix"], I["layout"], I["eot"], heads=R.TEXT_HEADS)
        dctx, ddeep = R.text_bwd_deep(sd, I["dfeat"], tctx)
        want, octx = O.text_encoder_fwd(sd, O.assemble_prompts(I["ctx"], I["prefix"], I["suffix"], I["layout"]), I["eot"], heads=R.TEXT_HEADS)
        want_d = O.scatter_prompt_grad(O.text_encoder_bwd(sd, I["dfeat"], octx), I["layout"], tuple(I["ctx"].shape))
    assert ddeep is None
    assert torch.equal(feat, want) and torch.equal(dctx, want_d)


def test_ctx_positions_match_the_layout(sd):
    for position in ("end", "middle", "front"):
        layout = O.build_prompt_layout(R.NAME_LENS, R.N_CTX, 20, position)
        cp = R.ctx_positions(layout, R.N_CTX)
        for c in range(len(R.NAME_LENS)):
            for j in range(R.N_CTX):
                assert int(layout[c, cp[c, j]]) == -(j + 1)


@pytest.mark.parametrize("n_deep", [1, 2, 3])
def test_deep_prompts_move_the_features_far_beyond_the_bar(sd, n_deep):
    """The scale of the test's ctx_deep values (R.CTX_DEEP_STD) is large enough for a no-op to be seen: features with and without the
    deep prompts differ by more than 10 x the bar (the logits of a whole step: tests/test_hip_deep_text.py, on the same figures)."""
    I = R.text_inputs(77, "end", n_deep)
    with torch.no_grad():
        a, _ = R.text_fwd_deep(sd, I["ctx"], I["ctx_deep"], I["prefix"], I["suffix"], I["layout"], I["eot"], heads=R.TEXT_HEADS, need_bwd=False)
        b, _ = R.text_fwd_deep(sd, I["ctx"], None, I["prefix"], I["suffix"], I["layout"], I["eot"], heads=R.TEXT_HEADS, need_bwd=False)
    d = rel(a, b)
    print(f"n_deep {n_deep}: features with / without deep prompts differ by {d:.3e}")
    assert d > 10 * BAR
