"""The ResNet image tower on the HIP engine (-m gpu): the four feature fixtures of the REAL reference (tools/make_resnet_golden.py) at the
project's tower bar (features within 1e-3 max|ref|, logits within 1e-3 of max(1, max|ref|) and allclose(rtol = atol = 1e-3), grad_ctx
within 1e-3 of its max), batch independence, determinism, the shared workspace, the refusals, and the trainers that reach a ResNet
(CoOp through the MVLPT trainer with VPT.N_CTX 0, CoCoOp, zero-shot, feature extraction for the linear probe).

The feature tests also print the device's distance to the fp16-rounding emulation (tests/resnet_ref.py round16=True) for the two small
cases: a diagnostic of the accumulation order, not an assertion."""
import numpy as np
import pytest
import torch

from tests import resnet_ref as R
from tests.golden_util import load_npz, t
from tests.test_resnet_ref import FEATURE_CASES, IDS, case_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-3            # tests/test_hip_model.py TOL_FP16, tests/test_hip_zsclip.py TOL


def _rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max()) / float(ref.abs().max())


def _check_logits(logits, ref, what):
    logits, ref = logits.detach().float().cpu(), t(ref)
    err = float((logits - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    print(f"{what}: logits err {err:.3e}")
    assert err < TOL, f"{what}: logits err {err:.3e} (relative to max(1, max|ref|))"
    assert torch.allclose(logits, ref, rtol=TOL, atol=TOL), f"{what}: logits element-wise allclose failed"


@pytest.fixture(scope="module")
def tiny():
    """(FrozenCLIP on tiny-rn with the fixtures' weights, its state dict)."""
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    sd = make_state_dict(RESNET_ARCHS["tiny-rn"], 1, include_token_embedding=True)
    return FrozenCLIP(sd, compute_dtype="fp16", device=DEV), sd


def tiny_images(B, seed=0):
    return torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ------------------------------------------------------------------------------------------------ features
@pytest.mark.parametrize("case,name", list(zip(FEATURE_CASES, IDS)), ids=IDS)
def test_features_match_the_reference(case, name):
    from mvlpt_amd.model import FrozenCLIP
    arch, sd, image, z = case_inputs(*case)
    clip = FrozenCLIP(sd, compute_dtype="fp16", device=DEV, arch=arch)
    assert clip.engine.resnet and clip.arch.embed_dim == z["features"].shape[1]
    feat = clip.encode_image(image)
    torch.cuda.synchronize()
    assert feat.shape == z["features"].shape and feat.dtype == torch.float32
    err = _rel(feat, z["features"])
    msg = f"{name}: features err {err:.3e} of max|ref|"
    if name.startswith("tiny"):
        emulated = R.resnet_features(sd, image, arch.vision_layers, round16=True)
        msg += f"; device vs fp16-rounding emulation {_rel(feat, emulated):.3e}"
    print(msg)
    assert err <= TOL, msg


def test_batch_rows_do_not_depend_on_the_batch(tiny):
    """Every output pixel of a convolution accumulates its K terms in the same order wherever its tile sits, so the convolutional
    part is bit-equal; the attention-pool projections run on GEMM kernels chosen by M.  Asserted: within 1e-6 max; printed: whether
    the rows came out bit-equal."""
    clip, _ = tiny
    image = tiny_images(5, 1)
    whole = clip.encode_image(image).cpu()
    rows = torch.cat([clip.encode_image(image[i:i + 1]).cpu() for i in range(5)])
    print("B = 1 rows bit-equal to the batched rows:", torch.equal(whole, rows))
    assert float((whole - rows).abs().max()) <= 1e-6 * float(whole.abs().max())


def test_two_calls_are_bit_equal(tiny):
    clip, _ = tiny
    image = tiny_images(4, 2)
    a = clip.encode_image(image).cpu()
    b = clip.encode_image(image).cpu()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def _text_step(clip, sd):
    """One text forward + backward on the engine (5 classes, 4 context tokens)."""
    from mvlpt_amd.model import build_prompt_layout
    case = load_npz("tiny_rn_coop")
    eng = clip.engine
    layout = build_prompt_layout(case["name_lens"].tolist(), 4, 77, "end")
    eot = t(case["tokenized_prompts"]).argmax(-1).to(torch.int32)
    feat = eng.text_fwd(t(case["token_prefix"]).to(DEV), t(case["token_suffix"]).to(DEV), t(case["param_ctx"]).to(DEV), layout.to(DEV),
                        eot.to(DEV), save_for_bwd=True)
    return feat, eng.text_bwd(torch.ones_like(feat))


def test_text_tower_between_two_image_forwards(tiny):
    clip, sd = tiny
    image = tiny_images(3, 3)
    a = clip.encode_image(image).cpu()
    feat, dctx = _text_step(clip, sd)
    b = clip.encode_image(image).cpu()
    assert torch.equal(a, b)
    assert bool(torch.isfinite(feat).all()) and bool(torch.isfinite(dctx).all()) and float(dctx.abs().max()) > 0


def test_trim_then_forward(tiny):
    clip, _ = tiny
    small, large = tiny_images(2, 4), tiny_images(9, 5)
    a = clip.encode_image(small).cpu()
    clip.encode_image(large)                      # grows the workspace: the old block is retired
    clip.engine.trim()
    assert torch.equal(clip.encode_image(small).cpu(), a)


def test_refusals_leave_the_engine_usable(tiny):
    import ctypes as C
    from mvlpt_amd import _lib
    clip, _ = tiny
    eng, lib = clip.engine, _lib.lib
    image = tiny_images(2, 6)
    want = clip.encode_image(image).cpu()
    vpt = torch.zeros(2, 512, device=DEV)
    feat = torch.empty(2, 128, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    # the library, called directly
    U = _lib.ERR_UNSUPPORTED
    assert lib.mvlpt_image_fwd(eng.h, p(image), _lib.DT_F32, p(vpt), None, 2, 0, 2, p(feat), 0, st) == U
    assert "mvlpt.py:48" in _lib.last_error(eng.h)
    assert lib.mvlpt_image_fwd(eng.h, p(image), _lib.DT_F32, None, p(vpt), 0, 1, 2, p(feat), 0, st) == U
    assert lib.mvlpt_image_fwd(eng.h, p(image), _lib.DT_F32, None, None, 0, 0, 2, p(feat), 1, st) == U
    assert lib.mvlpt_image_bwd(eng.h, p(feat), None, None, st) == U
    assert lib.mvlpt_image_fwd_begin(eng.h, p(image), _lib.DT_F32, None, None, 0, 0, 2, 0, 1, st) == U
    assert lib.mvlpt_image_fwd_resume(eng.h, p(feat), st) == U
    assert lib.mvlpt_set_vpt_dropout(eng.h, p(vpt), 1, 2, 1, 512) == U
    for mode in ("fast", "split_all", "split_grad"):      # accepted; the tower runs single fp16 operands in each
        eng.set_precision(mode)
        assert torch.equal(clip.encode_image(image).cpu(), want)
    # the Python layer refuses before any device call
    for call in (lambda: eng.image_fwd(image, vpt=vpt), lambda: eng.image_fwd(image, save_for_bwd=True),
                 lambda: eng.image_fwd_begin(image), lambda: eng.image_fwd_resume(), lambda: eng.image_bwd(feat),
                 lambda: eng.set_vpt_dropout(torch.ones(1, 2, 1, 512, device=DEV))):
        with pytest.raises(ValueError, match="ResNet"):
            call()
    assert torch.equal(clip.encode_image(image).cpu(), want)


def test_bf16_is_refused():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import RESNET_ARCHS
    with pytest.raises(ValueError, match="fp16"):
        Engine(RESNET_ARCHS["tiny-rn"], "bf16", DEV)


def test_missing_tensor_is_named():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    sd = make_state_dict(RESNET_ARCHS["tiny-rn"], 1)
    del sd["visual.layer2.1.bn2.running_var"]
    with pytest.raises(RuntimeError, match=r"visual\.layer2\.1\.bn2\.running_var"):
        Engine.from_state_dict(sd, "fp16", DEV)


# ------------------------------------------------------------------------------------------------ CoOp
def _coop_cfg(n_ctx=4, vpt=0):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny-rn"
    cfg.INPUT.SIZE = (64, 64)
    cfg.TRAINER.MVLPT.COOP.N_CTX = n_ctx
    cfg.TRAINER.MVLPT.COOP.CLASS_TOKEN_POSITION = "end"
    cfg.TRAINER.MVLPT.VPT.N_CTX = vpt
    return cfg


def test_coop_matches_the_reference(tiny):
    """trainers/coop.py on tiny-rn: the MVLPT model with VPT.N_CTX 0 is the reference's CoOp."""
    from mvlpt_amd.model import CustomCLIP, PretokenizedPrompts
    clip, _ = tiny
    case = load_npz("tiny_rn_coop")
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist())
    model = CustomCLIP(_coop_cfg(), [str(c) for c in case["classnames"]], clip, pretokenized=pre)
    model.prompt_learner.load_state_dict({"ctx": t(case["param_ctx"]), "token_prefix": t(case["token_prefix"]),
                                          "token_suffix": t(case["token_suffix"])}, strict=True)
    model = model.to(DEV)
    assert not model.split_active()
    B = len(case["label"])
    image = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(int(case["image_seed"])))
    logits = model(image.to(DEV), task=None)
    loss = model.cross_entropy(logits, t(case["label"]).to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    _check_logits(logits, case["out_logits"], "tiny_rn_coop")
    assert abs(float(loss.detach()) - float(case["out_loss"])) < TOL
    g = _rel(model.prompt_learner.ctx.grad, case["grad_ctx"])
    print(f"tiny_rn_coop: loss {float(loss.detach()):.6f} (reference {float(case['out_loss']):.6f}), grad_ctx err {g:.3e} of its max")
    assert g < TOL


def _mvlpt_trainer(tmp_path, pipelining, monkeypatch=None):
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    cfg = _coop_cfg()
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.OPTIM.MAX_EPOCH = 1
    cfg.OPTIM.LR = 0.05
    cfg.OPTIM.WARMUP_EPOCH = 0
    cfg.TRAIN.PRINT_FREQ = 10 ** 9
    cfg.TRAINER.MVLPT.STEP_PIPELINING = pipelining
    dm = SyntheticDataManager(cfg, 5, 3, device="cuda", seed=3)
    return MVLPT(cfg, dm=dm)      # no state dict: the backbone name is looked up (get_arch) and the weights generated


def test_mvlpt_trainer_steps_with_and_without_pipelining(tmp_path, monkeypatch):
    monkeypatch.setenv("MVLPT_PREFETCH_SPLIT", "1:64")       # a split in the environment must stay inactive on a ResNet
    losses = []
    for pipe in (False, True):
        torch.manual_seed(0)
        tr = _mvlpt_trainer(tmp_path, pipe)
        assert tr.model.engine.resnet and not tr.model.split_active()
        tr.epoch = 0
        out = tr.run_epoch()                                # three batches through the real loop (the look-ahead prefetch when on)
        losses.append(float(out["loss"]))
        assert np.isfinite(losses[-1])
    assert losses[0] == losses[1], losses


def test_visual_prompts_on_a_resnet_raise(tmp_path):
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    cfg = _coop_cfg(vpt=4)
    cfg.OUTPUT_DIR = str(tmp_path)
    dm = SyntheticDataManager(cfg, 5, 1, device="cuda", seed=3)
    with pytest.raises(ValueError, match=r"trainers/mvlpt\.py:48"):
        MVLPT(cfg, dm=dm)
    # ... and with the weights passed in (the name is not consulted): the prompt learner refuses
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    cfg.MODEL.BACKBONE.NAME = "custom"
    with pytest.raises(ValueError, match=r"trainers/mvlpt\.py:48"):
        MVLPT(cfg, dm=dm, clip_state_dict=make_state_dict(RESNET_ARCHS["tiny-rn"], 1))


# ------------------------------------------------------------------------------------------------ CoCoOp, zero-shot, linear probe
def test_cocoop_matches_the_reference(tiny):
    from mvlpt_amd.cocoop import CustomCLIP
    from mvlpt_amd.model import PretokenizedPrompts
    from tests.test_cocoop_host import cocoop_cfg
    from tests.test_hip_cocoop import run_cocoop
    clip, _ = tiny
    case = load_npz("tiny_rn_cocoop")
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist())
    model = CustomCLIP(cocoop_cfg(case, 64), [str(c) for c in case["classnames"]], clip, pretokenized=pre)
    state = {k[len("param_"):]: t(v) for k, v in case.items() if k.startswith("param_")}
    state["token_prefix"], state["token_suffix"] = t(case["token_prefix"]), t(case["token_suffix"])
    model.prompt_learner.load_state_dict(state, strict=True)
    model = model.to(DEV)
    logits, loss, grads = run_cocoop(model, t(case["image"]).to(DEV), t(case["label"]).to(DEV))
    margins = {"logits": _rel(logits, case["out_logits"]),
               "loss": abs(float(loss) - float(case["out_loss"])) / max(1.0, abs(float(case["out_loss"])))}
    for k, g in grads.items():
        margins["grad " + k] = _rel(g, case["grad_" + k])
    print("tiny_rn_cocoop: " + ", ".join(f"{k} {v:.2e}" for k, v in margins.items()))
    _check_logits(logits, case["out_logits"], "tiny_rn_cocoop")
    bad = {k: v for k, v in margins.items() if not v <= TOL}
    assert not bad, f"outside 1e-3 of the reference: {bad}"


def test_zeroshot_matches_the_reference(tmp_path):
    from mvlpt_amd import zsclip
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import SyntheticDataManager
    case = load_npz("tiny_rn_zsclip")
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny-rn"
    cfg.INPUT.SIZE = (64, 64)
    cfg.SEED = 1                                                  # the fixture's weight seed: the trainer generates them by name
    cfg.TRAINER.NAME = "ZeroshotCLIP"
    cfg.TRAINER.ZSCLIP.TEMPLATES = [str(s) for s in case["templates"]]
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 3
    cfg.OUTPUT_DIR = str(tmp_path)
    names = [str(c) for c in case["classnames"]]
    dm = SyntheticDataManager(cfg, num_classes=len(names), steps_per_epoch=1, seed=3)
    dm.classnames = names
    tr = zsclip.ZeroshotCLIP(cfg, dm=dm)
    assert torch.equal(tr.tokenized_prompts, t(case["tokenized_prompts"]))
    assert float((tr.text_features.cpu() - t(case["text_features"])).abs().max()) <= TOL
    logits = tr.model_inference(t(case["image"]).to(DEV))
    _check_logits(logits, case["out_logits"], "tiny_rn_zsclip")


def test_extract_features_rows_are_encode_image_rows(tiny):
    from mvlpt_amd import linear_probe as LP
    clip, _ = tiny
    g = torch.Generator().manual_seed(0)
    sizes = [3, 1, 4]
    batches = [(torch.randn(b, 3, 64, 64, generator=g), torch.arange(b) + 10 * k) for k, b in enumerate(sizes)]
    feats, labels = LP.extract_features(clip, iter(batches))
    assert feats.shape == (sum(sizes), 128) and feats.dtype == np.float32 and labels.dtype == np.int64
    want = np.concatenate([clip.encode_image(im).cpu().numpy() for im, _ in batches])
    assert feats.tobytes() == want.tobytes()
