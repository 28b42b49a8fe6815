"""Image towers with heads wider than 64 (-m gpu, path level) on "tiny-h": 640 = 8 heads of 80, 10 tokens at 48 px.

The reference cannot describe such a tower (clip/model.py:268: heads = width // 64), so the expected values are computed at test time on the
CPU by oracle.clip_oracle with vision_heads = 8.  Prompts, labels and parameters are those of the existing fixtures (the text tower of
"tiny-h" has the dimensions of "tiny"); the image is drawn here at the tower's resolution.  Bar: the project's 1e-3 on logits, loss and
every prompt gradient, normalised as tests/test_hip_model.py normalises (its run_case does the comparison).

Covered: CoOp through mvlpt_amd.model.CustomCLIP (the MVLPT trainer's model) under QuickGELU and under the exact GELU of the real
ViT-H/14 checkpoints; CoCoOp and zero-shot logits; features at 144 px (82 tokens: two key chunks) in one piece and through
image_fwd_begin / _resume; batch independence; every refusal of the C ABI, after which the engine still runs."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.golden_util import case_grads, load_npz, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
RES = 48
HEADS = (8, 2)
COOP_CASE = "tiny_coop_end"


def _arch():
    from mvlpt_amd.weights import WIDE_HEAD_ARCHS
    return WIDE_HEAD_ARCHS["tiny-h"]


@pytest.fixture(scope="module")
def sd():
    from mvlpt_amd.weights import make_state_dict
    return make_state_dict(_arch(), 1, include_token_embedding=True)


@pytest.fixture(scope="module")
def clip(sd):
    from mvlpt_amd.model import FrozenCLIP
    c = FrozenCLIP(sd, compute_dtype="fp16", device=DEV, vision_head_width=80)
    assert dataclasses.replace(c.arch, name="tiny-h") == _arch() and c.arch.vision_heads == 8
    return c


def _image(B, res=RES, seed=11):
    return torch.randn(B, 3, res, res, generator=torch.Generator().manual_seed(seed))


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _frozen(sd):
    return {k: v for k, v in sd.items() if k != "token_embedding.weight"}


def _coop_want(sd, run_oracle):
    """the fixture COOP_CASE with its image replaced by one of the tower's resolution and its outputs by the oracle's on these weights"""
    case = load_npz(COOP_CASE)
    image = _image(case["out_logits"].shape[0])
    res, _ = run_oracle(case, _frozen(sd), image, t(case["token_prefix"]), t(case["token_suffix"]), *HEADS)
    want = {k: v for k, v in case.items() if not k.startswith("grad_")}
    want["out_logits"], want["out_loss"] = res.logits.numpy(), res.loss.numpy()
    assert set(res.grads) == set(case_grads(case)) == {"ctx"}
    for k, g in res.grads.items():
        want["grad_" + k] = g.numpy()
    return case, want, image


def _run_coop(clip, case, want, image):
    from tests.test_hip_model import build_model, run_case
    model = build_model(want, clip, RES, t(case["token_prefix"]), t(case["token_suffix"]))
    err, worst = run_case(want, model, image, BAR, BAR)
    return err, worst


def test_coop_matches_the_oracle_with_eight_heads(clip, sd):
    from tests.test_oracle_golden import run_oracle_on_case
    case, want, image = _coop_want(sd, run_oracle_on_case)
    err, worst = _run_coop(clip, case, want, image)
    print(f"tiny-h coop: logits {err:.2e} grad_ctx {worst['ctx']:.2e}")
    # ten heads of 64 over the same weights (what the reference's build_model would assume) are another function
    res10, _ = run_oracle_on_case(case, _frozen(sd), image, t(case["token_prefix"]), t(case["token_suffix"]), 10, 2)
    assert _rel(res10.logits, want["out_logits"]) > 10 * BAR, "the oracle does not tell 8 heads of 80 from 10 heads of 64 on these inputs"


def test_coop_under_the_exact_gelu(clip, sd):
    """activation = "gelu", the setting of the real ViT-H/14 checkpoints; the oracle's activation is replaced the way
    tests/test_hip_gelu_towers.py replaces it."""
    from tests.test_hip_gelu_towers import _GeluOracle
    from tests.test_oracle_golden import run_oracle_on_case
    quick = _coop_want(sd, run_oracle_on_case)[1]
    o = _GeluOracle()
    try:
        case, want, image = _coop_want(sd, run_oracle_on_case)
    finally:
        o.mp.undo()
    assert _rel(want["out_logits"], quick["out_logits"]) > BAR, "the replaced activation changed nothing in the oracle"
    clip.engine.set_activation("gelu")
    try:
        err, worst = _run_coop(clip, case, want, image)
    finally:
        clip.engine.set_activation("quick_gelu")
    print(f"tiny-h coop gelu: logits {err:.2e} grad_ctx {worst['ctx']:.2e}")


def test_cocoop_logits(clip, sd):
    from mvlpt_amd import _lib
    from mvlpt_amd.cocoop import CustomCLIP
    from mvlpt_amd.model import PretokenizedPrompts
    from tests.test_cocoop_host import cocoop_cfg, oracle_cocoop
    case = load_npz("tiny_cocoop")
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist())
    model = CustomCLIP(cocoop_cfg(case, RES), [str(c) for c in case["classnames"]], clip, pretokenized=pre)
    assert clip.engine.precision == _lib.PREC_SPLIT_GRAD, "CoCoOp raised a wide-headed tower to split operands"
    params = {k[len("param_"):]: t(v) for k, v in case.items() if k.startswith("param_")}
    model.prompt_learner.load_state_dict(dict(params, token_prefix=t(case["token_prefix"]), token_suffix=t(case["token_suffix"])), strict=True)
    assert np.array_equal(model.prompt_learner.layout.numpy(), case["layout"])
    model = model.to(DEV)
    image = _image(len(case["label"]), seed=12)
    want_logits, want_loss, _grads, _ = oracle_cocoop(_frozen(sd), params, image, t(case["label"]), t(case["token_prefix"]),
                                                      t(case["token_suffix"]), t(case["layout"]), t(case["eot"]), *HEADS)
    model.prompt_learner.eval()
    with torch.no_grad():
        logits = model(image.to(DEV))
    model.prompt_learner.train()
    loss = model(image.to(DEV), t(case["label"]).to(DEV))
    torch.cuda.synchronize()
    e_logits = float((logits.double().cpu() - want_logits.detach().double()).abs().max()) / max(1.0, float(want_logits.abs().max()))
    e_loss = abs(float(loss.detach()) - float(want_loss))
    print(f"tiny-h cocoop: logits {e_logits:.2e} loss {e_loss:.2e}")
    assert e_logits < BAR and e_loss < BAR


def test_zero_shot_logits(clip, sd):
    from oracle import clip_oracle as O
    ids = t(load_npz("tiny_zsclip")["tokenized_prompts"])
    image = _image(4, seed=13)
    txt = clip.engine.text_ensemble(clip.encode_text(ids)[None])
    scale = float(sd["logit_scale"].exp())
    logits = clip.engine.logits_fwd(clip.encode_image(image), txt, scale).cpu()
    with torch.no_grad():
        fz = _frozen(sd)
        want_img, _ = O.image_encoder_fwd(fz, image, None, None, heads=HEADS[0], need_bwd=False)
        want_txt, _ = O.text_encoder_fwd(fz, sd["token_embedding.weight"].float()[ids], ids.argmax(-1), heads=HEADS[1], need_bwd=False)
        want, _ = O.logits_fwd(want_img, want_txt, scale)
    err = float((logits.double() - want.double()).abs().max()) / max(1.0, float(want.abs().max()))
    print(f"tiny-h zero-shot: logits {err:.2e}")
    assert err < BAR


@pytest.fixture(scope="module")
def clip144():
    """the same tower at 144 px: 81 patches + CLS = 82 tokens, two key chunks"""
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import make_state_dict
    arch = dataclasses.replace(_arch(), name="tiny-h@144", image_resolution=144)
    sd = make_state_dict(arch, 4)
    return FrozenCLIP(sd, compute_dtype="fp16", device=DEV, arch=arch), sd


def test_features_at_82_tokens_in_one_piece_and_in_two(clip144):
    from oracle import clip_oracle as O
    c, sd = clip144
    eng = c.engine
    image = _image(3, 144, seed=14).to(DEV)
    whole = eng.image_fwd(image).clone()
    with torch.no_grad():
        want, _ = O.image_encoder_fwd(sd, image.cpu(), None, None, heads=8, need_bwd=False)
    err = _rel(whole, want)
    print(f"tiny-h@144 features: {err:.2e}")
    assert err < BAR
    for stop in (1, None, 0):
        eng.image_fwd_begin(image, stop_block=stop)
        assert eng.image_fwd_pending()
        assert torch.equal(eng.image_fwd_resume(), whole), stop
    eng.image_fwd_begin(image, stop_block=1)
    eng.image_fwd_abandon()
    assert not eng.image_fwd_pending() and torch.equal(eng.image_fwd(image), whole)
    # one image alone gives the bits of its row in the batch
    for b in range(3):
        assert torch.equal(eng.image_fwd(image[b:b + 1].contiguous())[0], whole[b]), b


def test_refusals_leave_the_engine_usable(clip):
    """visual prompts, save_for_bwd, mvlpt_image_bwd, mvlpt_set_vpt_dropout and MVLPT_PREC_SPLIT_ALL: MVLPT_ERR_UNSUPPORTED with the
    cause in the message; the forward before and after gives the same bits."""
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    lib, eng = _lib.lib, clip.engine
    h = eng.h
    image = _image(2, seed=15).to(DEV).half()
    before = eng.image_fwd(image).clone()
    dv, e = eng.arch.vision_width, eng.arch.embed_dim
    vpt = torch.zeros(2, dv, device=DEV)
    deep = torch.zeros(2, 2, dv, device=DEV)
    feat = torch.full((2, e), 7.0, device=DEV)
    dfeat = torch.zeros(2, e, device=DEV)
    dvpt = torch.zeros(2, dv, device=DEV)
    masks = torch.ones(1, 2, 2, dv, device=DEV)
    fwd = lambda v, d, nv, nd, save: lib.mvlpt_image_fwd(h, _ptr(image), _lib.DT_F16, _ptr(v), _ptr(d), nv, nd, 2, _ptr(feat), save, _stream())
    begin = lambda v, nv, save: lib.mvlpt_image_fwd_begin(h, _ptr(image), _lib.DT_F16, _ptr(v), None, nv, 0, 2, save, 1, _stream())
    calls = [("visual prompts", lambda: fwd(vpt, None, 2, 0, 0)), ("visual prompts", lambda: fwd(vpt, deep, 2, 2, 0)),
             ("save_for_bwd", lambda: fwd(None, None, 0, 0, 1)), ("visual prompts", lambda: begin(vpt, 2, 0)),
             ("save_for_bwd", lambda: begin(None, 0, 1)),
             ("image_bwd", lambda: lib.mvlpt_image_bwd(h, _ptr(dfeat), _ptr(dvpt), None, _stream())),
             ("set_vpt_dropout", lambda: lib.mvlpt_set_vpt_dropout(h, _ptr(masks), 1, 2, 2, dv))]
    for cause, call in calls:
        rc, msg = call(), _lib.last_error(h)
        assert rc == _lib.ERR_UNSUPPORTED and cause in msg and "heads wider than 64" in msg, (cause, rc, msg)
        assert not eng.image_fwd_pending()
    eng.set_precision("split_all")
    try:
        rc, msg = fwd(None, None, 0, 0, 0), _lib.last_error(h)
        assert rc == _lib.ERR_UNSUPPORTED and "MVLPT_PREC_SPLIT_ALL" in msg and "heads wider than 64" in msg, (rc, msg)
    finally:
        eng.set_precision("split_grad")
    torch.cuda.synchronize()
    assert bool((feat == 7.0).all()), "a refused call wrote its output"
    assert torch.equal(eng.image_fwd(image), before)
    eng.set_precision("fast")
    try:
        assert torch.equal(eng.image_fwd(image), before)      # single operands in this mode too
    finally:
        eng.set_precision("split_grad")
