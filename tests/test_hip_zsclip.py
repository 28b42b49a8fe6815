"""Zero-shot CLIP on the HIP engine (-m gpu): the token-id text route against the existing prefix / suffix route (bit for bit), trimming
and chunking, the three fixtures of the REAL reference (tools/make_zsclip_golden.py) at the project's inference criterion
(tests/test_hip_model.py: logits within 1e-3, features within 1e-3 max|ref|), the two trainers, and the shared workspace afterwards.

The fixture test prints the logits error and the largest absolute error of text_features; DESIGN.md §2 is where measured figures go
(none recorded yet)."""
import numpy as np
import pytest
import torch

from tests.golden_util import load_npz, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-3            # the bound of the 18 existing inference fixtures (tests/test_hip_model.py TOL_FP16)
FIXTURES = ["tiny_zsclip", "tiny_zsclip_ensemble", "full_vitb16_zsclip"]


def _clip(name, cache={}):
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    key = "tiny" if name.startswith("tiny") else "ViT-B/16"
    if key not in cache:
        cache.clear()
        sd = make_state_dict(ARCHS[key], 1 if key == "tiny" else 2, include_token_embedding=True)
        cache[key] = (FrozenCLIP(sd, compute_dtype="fp16", device=DEV), sd)      # the mode the other full_* inference tests use
    return cache[key]


def _feat_err(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((a - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ the new assembly
@pytest.mark.parametrize("L", [77, 20])
def test_token_route_is_bit_identical_to_the_prefix_suffix_route(L):
    clip, sd = _clip("tiny")
    case = load_npz("tiny_zsclip_ensemble")
    ids = t(case["tokenized_prompts"])
    assert int(ids.argmax(-1).max()) < L
    clip.encode_text(ids[:1])                                     # uploads the token embedding
    got = clip.engine.text_encode_tokens(ids, L)
    emb = sd["token_embedding.weight"].float()[ids[:, :L]]        # the CPU lookup the prompt-tuning routes start from
    S = ids.shape[0]
    layout = torch.arange(L, dtype=torch.int32).repeat(S, 1)      # position 0 = prefix, i > 0 = suffix row i - 1
    want = clip.engine.text_fwd(emb[:, :1].contiguous().to(DEV), emb[:, 1:].contiguous().to(DEV), None, layout.to(DEV),
                                ids.argmax(-1).to(torch.int32).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got, want), "same tower, same input bits: any difference is the new assembly"


# ------------------------------------------------------------------------------------------------ trimming and chunking
@pytest.fixture()
def ensemble_case():
    clip, _ = _clip("tiny")
    saved = (clip.max_text_workspace_bytes, clip.min_sequences_per_chunk)
    yield clip, load_npz("tiny_zsclip_ensemble")
    clip.max_text_workspace_bytes, clip.min_sequences_per_chunk = saved


def test_trimmed_buckets_against_the_full_context_length(ensemble_case):
    clip, case = ensemble_case
    ids, ref = t(case["tokenized_prompts"]), t(case["text_features_per_template"]).flatten(0, 1)
    assert len(set(ids.argmax(-1).tolist())) >= 3
    clip.min_sequences_per_chunk = 1                              # one chunk per prompt length
    trimmed = clip.encode_text(ids).cpu()
    plan = list(clip.last_text_chunks)
    assert len(plan) >= 3 and sum(n for _, n in plan) == ids.shape[0] and len({L for L, _ in plan}) == len(plan)
    full = clip.encode_text(ids, trim=False).cpu()
    assert clip.last_text_chunks == [(77, ids.shape[0])]
    e_trim, e_full, e_mutual = _feat_err(trimmed, ref), _feat_err(full, ref), _feat_err(trimmed, full)
    print(f"trimmed {e_trim:.3e} full {e_full:.3e} mutual {e_mutual:.3e} chunks {plan}")
    assert e_trim <= TOL and e_full <= TOL
    assert float((trimmed - full).abs().max()) <= 2 * TOL * float(ref.abs().max())


def test_a_small_workspace_budget_forces_chunks(ensemble_case):
    clip, case = ensemble_case
    ids, ref = t(case["tokenized_prompts"]), t(case["text_features_per_template"]).flatten(0, 1)
    n, L = ids.shape[0], int(ids.argmax(-1).max()) + 1
    one = clip.encode_text(ids).cpu()
    assert clip.last_text_chunks == [(L, n)]
    clip.max_text_workspace_bytes = clip.engine.text_encode_workspace_bytes(n // 3, L)
    a = clip.encode_text(ids).cpu()
    assert len(clip.last_text_chunks) >= 3
    b = clip.encode_text(ids).cpu()
    assert torch.equal(a, b)
    assert float((a - one).abs().max()) <= TOL * float(ref.abs().max())
    clip.max_text_workspace_bytes = clip.engine.text_encode_workspace_bytes(1, 3) - 1
    with pytest.raises(ValueError):
        clip.encode_text(ids)


# ------------------------------------------------------------------------------------------------ the reference's fixtures
def _fixture_image(case, res):
    if "image" in case:
        return t(case["image"])
    g = torch.Generator().manual_seed(int(case["image_seed"]))
    return torch.randn(int(case["image_batch"]), 3, res, res, generator=g)


def _check_logits(logits, case, name):
    ref = t(case["out_logits"])
    err = float((logits - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    assert err < TOL, f"{name}: logits err {err:.3e} (relative to max(1, max|ref|))"
    assert torch.allclose(logits, ref, rtol=TOL, atol=TOL), f"{name}: logits element-wise allclose failed"
    return err


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_logits(name):
    clip, _ = _clip(name)
    case = load_npz(name)
    T, C = len(case["templates"]), len(case["classnames"])
    feats = clip.encode_text(t(case["tokenized_prompts"]))
    txt = clip.engine.text_ensemble(feats.view(T, C, -1))
    img = clip.encode_image(_fixture_image(case, clip.arch.image_resolution))
    logits = clip.engine.logits_fwd(img, txt, float(np.exp(case["logit_scale"]))).cpu()
    err = _check_logits(logits, case, name)
    txt_err = float((txt.cpu() - t(case["text_features"])).abs().max())
    print(f"{name}: logits err {err:.3e}, max |text_features - ref| {txt_err:.3e}, "
          f"per-template features {_feat_err(feats, t(case['text_features_per_template']).flatten(0, 1)):.3e}")


# ------------------------------------------------------------------------------------------------ trainers
def _trainer(cls_name, case, tmp_path):
    from mvlpt_amd import zsclip
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import SyntheticDataManager
    from mvlpt_amd.weights import ARCHS, make_state_dict
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.TRAINER.NAME = cls_name
    cfg.TRAINER.ZSCLIP.TEMPLATES = [str(s) for s in case["templates"]]
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 3
    cfg.OUTPUT_DIR = str(tmp_path)
    names = [str(c) for c in case["classnames"]]
    dm = SyntheticDataManager(cfg, num_classes=len(names), steps_per_epoch=1, seed=3)
    dm.classnames = names
    best = t(case["out_logits"]).argmax(1)
    label = best.clone()
    label[-1] = (label[-1] + 1) % len(names)                      # the last image counts as a miss
    dm.test_loader = [{"img": t(case["image"]), "label": label, "domain": torch.zeros(len(label), dtype=torch.long)}]
    sd = make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True)
    return getattr(zsclip, cls_name)(cfg, dm=dm, clip_state_dict=sd), label


@pytest.mark.parametrize("cls_name,name", [("ZeroshotCLIP", "tiny_zsclip"), ("ZeroshotCLIP2", "tiny_zsclip_ensemble")])
def test_trainers_reproduce_the_reference(cls_name, name, tmp_path):
    case = load_npz(name)
    tr, label = _trainer(cls_name, case, tmp_path)
    assert torch.equal(tr.tokenized_prompts, t(case["tokenized_prompts"]))
    assert tr.text_features.shape == case["text_features"].shape
    assert float((tr.text_features.cpu() - t(case["text_features"])).abs().max()) <= TOL
    logits = tr.model_inference(t(case["image"]).to(DEV)).cpu()
    _check_logits(logits, case, name)
    want = 100.0 * float((t(case["out_logits"]).argmax(1) == label).sum()) / len(label)
    assert tr.test() == pytest.approx(want)
    assert 0.0 < want < 100.0
    tr.build_model()                                              # a second build neither grows nor changes the templates
    assert tr.templates == [str(s) for s in case["templates"]]
    if cls_name == "ZeroshotCLIP":
        from mvlpt_amd import zsclip
        tr.cfg.TRAINER.ZSCLIP.TEMPLATES = ["a {}.", "the {}."]
        with pytest.raises(ValueError):
            zsclip.ZeroshotCLIP.build_model(tr)


# ------------------------------------------------------------------------------------------------ shared workspace
def test_the_token_route_leaves_no_state_in_the_text_workspace():
    from mvlpt_amd.model import FrozenCLIP, build_prompt_layout
    from mvlpt_amd.weights import ARCHS, make_state_dict
    used, sd = _clip("tiny")
    case = load_npz("tiny_zsclip_ensemble")
    ids = t(case["tokenized_prompts"])
    txt = used.engine.text_ensemble(used.encode_text(ids).view(8, 5, -1))
    used.engine.logits_fwd(used.encode_image(t(case["image"])), txt, 10.0)
    g = torch.Generator().manual_seed(11)
    C, L, n, dt = 5, 77, 4, used.arch.transformer_width
    layout = build_prompt_layout([1, 2, 2, 1, 3], n, L, "end").to(DEV)
    eot = torch.tensor([8, 9, 9, 8, 10], dtype=torch.int32, device=DEV)
    prefix = (torch.randn(C, 1, dt, generator=g) * 0.02).to(DEV)
    suffix = (torch.randn(C, L - 1 - n, dt, generator=g) * 0.02).to(DEV)
    ctx = (torch.randn(n, dt, generator=g) * 0.1).to(DEV)
    dfeat = torch.randn(C, used.arch.embed_dim, generator=g).to(DEV)
    outs = []
    for clip in (used, FrozenCLIP(sd, compute_dtype="fp16", device=DEV)):
        f = clip.engine.text_fwd(prefix, suffix, ctx, layout, eot, save_for_bwd=True)
        d = clip.engine.text_bwd(dfeat)
        torch.cuda.synchronize()
        outs.append((f.cpu(), d.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
