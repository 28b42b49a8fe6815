"""The towers under MVLPT_ACT_GELU (-m gpu, path level): checkpoints of CLIP's architecture whose MLPs were trained with nn.GELU.

Expected values are computed at test time on the CPU by oracle.clip_oracle with its two module-level functions quick_gelu /
quick_gelu_grad replaced (pytest's MonkeyPatch) by F.gelu and its derivative; the weights and inputs are those of the existing fixtures.
The prompt learner's own projection block (UPT, oracle.upt_project) is the reference's code, not the checkpoint's: it keeps QuickGELU on
both sides.  Bounds: the project's bar of 1e-3 on logits, loss and every prompt gradient, normalised as tests/test_hip_model.py
normalises (its run_case does the comparison).

Covered routes: block_fwd / block_bwd and the compact last blocks of both towers in the default precision mode (mixed pairs where a
gradient flows, single operands elsewhere) and in MVLPT_PREC_SPLIT_ALL (hi|lo pairs); the ranged text tower (CoCoOp); activation
checkpointing (recomputation in the backward); mvlpt_text_encode_tokens; and, on one full-size fixture, the rows of the padded pitch
between the two MLP GEMMs together with a folded ln_1 (LayerNorm folding forced on; under the exact GELU ln_2 is not folded)."""
import types

import numpy as np
import pytest
import torch

from tests.golden_util import case_grads, load_npz, t, tiny_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
MVLPT_CASES = ["tiny_coop_end", "tiny_coop_middle", "tiny_vpt_deep", "tiny_upt"]
FULL_CASE = ("ViT-B/32", "full_vitb32_coop_end")
# The recorded QuickGELU logits of these fixtures lie more than 10 x BAR from the GELU logits of the SAME weights and inputs by the
# oracle's own figures (1.6e-2 / 1.8e-2; the other tiny cases: 5.6e-3 .. 7.8e-3, too close to tell the two functions apart this way)
NOOP_GUARD_CASES = ["tiny_upt", "full_vitb32_coop_end"]


def _gelu_grad(u):
    return 0.5 * torch.erfc(-u * 0.7071067811865476) + u * (0.3989422804014327 * torch.exp(-0.5 * u * u))


class _GeluOracle:
    """oracle.clip_oracle with the towers' activation replaced, for the lifetime of the module's tests."""

    def __init__(self):
        from oracle import clip_oracle as O
        self.mp = pytest.MonkeyPatch()
        # the projection of the prompt learner keeps the reference's QuickGELU: the same function body over globals that still hold it
        keep = types.FunctionType(O.upt_project.__code__, {**O.__dict__, "quick_gelu": O.quick_gelu}, "upt_project")
        self.mp.setattr(O, "upt_project", keep)
        self.mp.setattr(O, "quick_gelu", lambda u: torch.nn.functional.gelu(u))
        self.mp.setattr(O, "quick_gelu_grad", _gelu_grad)
        self.O = O
        self.cache = {}

    def mvlpt(self, name, sd, image, prefix, suffix, heads):
        """the fixture `name` with its outputs and gradients replaced by the GELU oracle's"""
        if name not in self.cache:
            from tests.test_oracle_golden import run_oracle_on_case
            case = load_npz(name)
            res, _ = run_oracle_on_case(case, sd, image, prefix, suffix, *heads)
            want = {k: v for k, v in case.items() if not k.startswith("grad_")}
            want["out_logits"], want["out_loss"] = res.logits.numpy(), res.loss.numpy()
            assert set(res.grads) == set(case_grads(case))
            for k, g in res.grads.items():
                want["grad_" + k] = g.numpy()
            self.cache[name] = (case, want)
        return self.cache[name]


@pytest.fixture(scope="module")
def oracle():
    o = _GeluOracle()
    yield o
    o.mp.undo()


@pytest.fixture(scope="module")
def clips():
    """tiny frozen CLIPs under the exact GELU: the default precision mode and MVLPT_PREC_SPLIT_ALL"""
    from mvlpt_amd.model import FrozenCLIP
    return {"split_grad": FrozenCLIP(tiny_state_dict(), compute_dtype="fp16", activation="gelu"),
            "split_all": FrozenCLIP(tiny_state_dict(), compute_dtype="fp16", precision="split_all", activation="gelu")}


@pytest.fixture(scope="module")
def token_clip():
    """the tiny CLIP of the CoCoOp and zero-shot fixtures (seed 1, with its token embedding) under the exact GELU"""
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    sd = make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True)
    return FrozenCLIP(sd, compute_dtype="fp16", device=DEV, activation="gelu"), sd


def _logit_gap(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _run_tiny(name, clip, oracle, act_ckpt=1):
    from tests.test_hip_model import build_model, run_case
    sd = tiny_state_dict()
    case0 = load_npz(name)
    case, want = oracle.mvlpt(name, sd, t(case0["image"]), t(case0["token_prefix"]), t(case0["token_suffix"]), (2, 2))
    model = build_model(want, clip, 32, t(case["token_prefix"]), t(case["token_suffix"]))
    clip.engine.set_text_act_ckpt(act_ckpt)      # (building a model sets TRAINER.ACT_CKPT, 1, on its engine)
    err, worst = run_case(want, model, t(case["image"]), BAR, BAR)
    print(f"{name} gelu: logits {err:.2e} grads {max(worst.values()):.2e}")
    return case, want, model


@pytest.mark.parametrize("precision", ["split_grad", "split_all"])
@pytest.mark.parametrize("name", MVLPT_CASES)
def test_mvlpt_case_under_gelu(name, precision, clips, oracle):
    clip = clips[precision]
    assert clip.engine.get_activation() == "gelu"
    case, want, model = _run_tiny(name, clip, oracle)
    if name in NOOP_GUARD_CASES:      # a silent no-op would reproduce the fixture's QuickGELU logits
        model.eval()
        with torch.no_grad():
            logits = model(t(case["image"]).to(clip.device)).cpu()
        assert _logit_gap(logits, t(case["out_logits"])) > 10 * BAR, "the gelu logits are the fixture's QuickGELU logits"


def test_switching_back_reproduces_the_fixtures(clips):
    """set_activation("quick_gelu") after gelu steps: the fixture's own expected values at the existing tolerance, and gelu again after."""
    from tests.test_hip_model import GRAD_TOL_FP16, TOL_TINY_FP16, build_model, run_case
    clip = clips["split_grad"]
    eng = clip.engine
    eng.set_activation("quick_gelu")
    try:
        assert eng.get_activation() == "quick_gelu"
        for name in ("tiny_coop_middle", "tiny_upt"):
            case = load_npz(name)
            model = build_model(case, clip, 32, t(case["token_prefix"]), t(case["token_suffix"]))
            run_case(case, model, t(case["image"]), TOL_TINY_FP16, GRAD_TOL_FP16)
    finally:
        eng.set_activation("gelu")
    assert eng.get_activation() == "gelu"


def test_activation_checkpointing_under_gelu(clips, oracle):
    """set_text_act_ckpt(2): the first text block is recomputed inside the backward, through the stand-alone pass and its scratch."""
    eng = clips["split_grad"].engine
    try:
        _run_tiny("tiny_coop_middle", clips["split_grad"], oracle, act_ckpt=2)
        assert [c for _, _, c in eng.text_act_ckpt_plan()] == [True, False]
    finally:
        eng.set_text_act_ckpt(1)


def test_cocoop_case_under_gelu(token_clip, oracle):
    """CoCoOp (ranged text tower, PREC_SPLIT_ALL as its CustomCLIP sets it) against trainers/cocoop.py restated on the GELU oracle
    (tests/test_cocoop_host.py: oracle_cocoop), with the parameters and inputs of the reference's fixture."""
    from mvlpt_amd.cocoop import CustomCLIP
    from mvlpt_amd.model import PretokenizedPrompts
    from tests.test_cocoop_host import cocoop_cfg, oracle_cocoop
    from tests.test_hip_cocoop import run_cocoop
    clip, sd = token_clip
    arch = clip.arch
    case = load_npz("tiny_cocoop")
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist())
    model = CustomCLIP(cocoop_cfg(case, arch.image_resolution), [str(c) for c in case["classnames"]], clip, pretokenized=pre)
    params = {k[len("param_"):]: t(v) for k, v in case.items() if k.startswith("param_")}
    model.prompt_learner.load_state_dict(dict(params, token_prefix=t(case["token_prefix"]), token_suffix=t(case["token_suffix"])), strict=True)
    assert np.array_equal(model.prompt_learner.layout.numpy(), case["layout"])
    model = model.to(DEV)
    frozen = {k: v for k, v in sd.items() if k != "token_embedding.weight"}
    want_logits, want_loss, want_grads, _ = oracle_cocoop(frozen, params, t(case["image"]), t(case["label"]), t(case["token_prefix"]),
                                                          t(case["token_suffix"]), t(case["layout"]), t(case["eot"]),
                                                          arch.vision_heads, arch.transformer_heads)
    assert clip.engine.get_activation() == "gelu"
    logits, loss, grads = run_cocoop(model, t(case["image"]).to(DEV), t(case["label"]).to(DEV))
    rel = lambda a, b: float((a.double().cpu() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)
    margins = {"logits": rel(logits, want_logits.detach()), "loss": abs(float(loss) - float(want_loss)) / max(1.0, abs(float(want_loss)))}
    for k, g in grads.items():
        margins["grad " + k] = rel(g, want_grads[k])
    print("tiny_cocoop gelu: " + ", ".join(f"{k} {v:.2e}" for k, v in margins.items()))
    assert len(grads) == 5 and not {k: v for k, v in margins.items() if not v <= BAR}, margins


def test_zero_shot_encode_text_under_gelu(token_clip, oracle):
    """mvlpt_text_encode_tokens (the zero-shot trainers' encode_text) against the oracle's text encoder on the same token ids."""
    clip, sd = token_clip
    ids = t(load_npz("tiny_zsclip")["tokenized_prompts"])
    got = clip.encode_text(ids).cpu()
    with torch.no_grad():
        want, _ = oracle.O.text_encoder_fwd({k: v for k, v in sd.items() if k != "token_embedding.weight"},
                                            sd["token_embedding.weight"].float()[ids], ids.argmax(-1), heads=clip.arch.transformer_heads)
    err = float((got.double() - want.double()).abs().max()) / float(want.abs().max())
    print(f"encode_text gelu: features {err:.2e}")
    assert err < BAR
    clip.engine.set_activation("quick_gelu")
    try:
        quick = clip.encode_text(ids).cpu()
    finally:
        clip.engine.set_activation("gelu")
    assert float((quick.double() - want.double()).abs().max()) / float(want.abs().max()) > BAR, "the setting changed nothing"


def test_full_size_case_with_padded_pitch_and_folded_ln1(oracle):
    """ViT-B/32 widths: the rows between the two MLP GEMMs get the padded pitch (4 width * 4 bytes is a multiple of 4 KiB) and, with
    LayerNorm folding forced on at these row counts, the down-projection behind the stand-alone pass produces the folded ln_1 input of
    the next block; ln_2 runs as a pass of its own.  Training forward + backward, and the silent-no-op guard."""
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    from tests.golden_util import full_case_inputs
    from tests.test_hip_model import build_model, run_case
    arch_name, name = FULL_CASE
    arch = ARCHS[arch_name]
    sd = make_state_dict(arch, 2, include_token_embedding=True)
    case0 = load_npz(name)
    image, pre, suf = full_case_inputs(case0, sd, arch.image_resolution)
    case, want = oracle.mvlpt(name, sd, image, pre, suf, (arch.vision_heads, arch.transformer_heads))
    clip = FrozenCLIP(sd, compute_dtype="fp16", activation="gelu")
    clip.engine.set_ln_fold(2, 1)
    model = build_model(want, clip, arch.image_resolution, pre, suf)
    err, worst = run_case(want, model, image, BAR, BAR)
    print(f"{name} gelu, folding forced: logits {err:.2e} grads {max(worst.values()):.2e}")
    model.eval()
    with torch.no_grad():
        logits = model(image.to(clip.device)).cpu()
    assert _logit_gap(logits, t(want["out_logits"])) < BAR
    assert _logit_gap(logits, t(case["out_logits"])) > 10 * BAR, "the gelu logits are the fixture's QuickGELU logits"


def _text_inputs(eng, C=5, L=77, n=4, seed=3):
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(seed)
    dt = eng.arch.transformer_width
    name_lens = ([1, 2, 2, 1, 3] * 4)[:C]
    layout = build_prompt_layout(name_lens, n, L, "end").to(DEV)
    eot = torch.tensor([n + k + 2 for k in name_lens], dtype=torch.int32, device=DEV)
    prefix = (torch.randn(C, 1, dt, generator=g) * 0.02).to(DEV)
    suffix = (torch.randn(C, L - 1 - n, dt, generator=g) * 0.02).to(DEV)
    ctx = (torch.randn(n, dt, generator=g) * 0.1).to(DEV)
    dfeat = torch.randn(C, eng.arch.embed_dim, generator=g).to(DEV)
    return (prefix, suffix, ctx, layout, eot), dfeat


def test_workspace_grows_by_the_documented_scratch_only_under_gelu(clips):
    """mvlpt_text_workspace_bytes: under gelu one fp32 [C L, 4 width] buffer for the tower and [C, 4 width] for the compact last block,
    each rounded up to 256 bytes; under quick_gelu the published figure is what it was."""
    eng = clips["split_grad"].engine
    d = eng.arch.transformer_width
    r256 = lambda b: (b + 255) // 256 * 256
    try:
        for C, L, save in ((5, 77, True), (5, 77, False), (3, 20, True), (1, 3, False)):
            eng.set_activation("gelu")
            with_scratch = eng.text_workspace_bytes(C, L, save)
            eng.set_activation("quick_gelu")
            without = eng.text_workspace_bytes(C, L, save)
            assert with_scratch - without == r256(C * L * 4 * d * 4) + r256(C * 4 * d * 4), (C, L, save)
    finally:
        eng.set_activation("gelu")


def test_set_activation_between_forward_and_backward_is_a_state_error(clips):
    from mvlpt_amd import _lib
    eng = clips["split_grad"].engine
    args, dfeat = _text_inputs(eng)
    eng.text_fwd(*args, save_for_bwd=True)
    want = eng.text_bwd(dfeat).clone()
    feat = eng.text_fwd(*args, save_for_bwd=True).clone()
    with pytest.raises(RuntimeError, match="set_activation"):
        eng.set_activation("quick_gelu")
    assert _lib.lib.mvlpt_set_activation(eng.h, _lib.ACT_QUICKGELU) == _lib.ERR_STATE and "backward has not run" in _lib.last_error(eng.h)
    assert eng.get_activation() == "gelu" and eng.activation == "gelu"
    got = eng.text_bwd(dfeat)
    torch.cuda.synchronize()
    assert torch.equal(got, want), "the backward behind a refused set_activation differs from an undisturbed one"
    # a completed step: the setting is legal again; unknown values are refused without a change
    eng.set_activation("quick_gelu")
    other = eng.text_fwd(*args)
    assert not torch.equal(other, feat)
    assert _lib.lib.mvlpt_set_activation(eng.h, 2) == _lib.ERR_ARG and _lib.lib.mvlpt_set_activation(eng.h, -1) == _lib.ERR_ARG
    assert eng.get_activation() == "quick_gelu"
    with pytest.raises(ValueError, match="'quick_gelu' and 'gelu'"):
        eng.set_activation("relu")
    eng.set_activation("gelu")
    assert torch.equal(eng.text_fwd(*args), feat)


def test_image_begin_resume_inherit_the_setting_and_refuse_a_change_in_between(clips):
    """mvlpt_image_fwd_begin / _resume under gelu: the bits of the one-piece forward on both sides of the cut, set_activation refused
    while the forward is pending and between a saving image forward and its backward."""
    eng = clips["split_grad"].engine
    g = torch.Generator().manual_seed(5)
    image = torch.randn(3, 3, 32, 32, generator=g).to(DEV)
    vpt = (torch.randn(2, eng.arch.vision_width, generator=g) * 0.1).to(DEV)
    dfeat = torch.randn(3, eng.arch.embed_dim, generator=g).to(DEV)
    whole = eng.image_fwd(image).clone()
    for stop in (1, None):
        eng.image_fwd_begin(image, stop_block=stop)
        with pytest.raises(RuntimeError, match="set_activation"):
            eng.set_activation("quick_gelu")
        assert torch.equal(eng.image_fwd_resume(), whole), stop
    eng.image_fwd(image, vpt, save_for_bwd=True)
    want = eng.image_bwd(dfeat)[0].clone()
    eng.image_fwd(image, vpt, save_for_bwd=True)
    with pytest.raises(RuntimeError, match="set_activation"):
        eng.set_activation("quick_gelu")
    assert torch.equal(eng.image_bwd(dfeat)[0], want)
    eng.set_activation("quick_gelu")
    try:
        assert not torch.equal(eng.image_fwd(image), whole)
    finally:
        eng.set_activation("gelu")
