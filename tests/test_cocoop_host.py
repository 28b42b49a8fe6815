"""CoCoOp (trainers/cocoop.py) host side, CPU only: the PromptLearner's checkpoint keys, buffers, integer tables and ctx-init against
fixtures generated through the REAL reference (tools/make_cocoop_golden.py), and the CPU oracle (oracle.clip_oracle encoders, used
read-only) run with the fixtures' parameters against their logits, loss and gradients (this pins the fixtures)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN, load_npz, t

TINY_COCOOP_CASES = ["tiny_cocoop", "tiny_cocoop_ctxinit"]


def cocoop_cfg(case, image_size):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.TRAINER.COCOOP.N_CTX = int(case["meta_n_ctx_cfg"])
    cfg.TRAINER.COCOOP.CTX_INIT = str(case["meta_ctx_init"])
    cfg.TRAINER.COCOOP.PREC = "fp32"
    cfg.INPUT.SIZE = (image_size, image_size)
    return cfg


def tiny_sd_with_tokens():
    from mvlpt_amd.weights import ARCHS, make_state_dict
    return make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True)      # oracle/make_golden.py TINY_SEED: tiny_clip.npz


def host_prompt_learner(case, sd):
    """The PromptLearner built on the oracle-backed frozen CLIP, with the real BPE tokenizer and the fixture's class names."""
    from mvlpt_amd.cocoop import PromptLearner
    from mvlpt_amd.model import default_tokenizer
    from mvlpt_amd.weights import ARCHS
    from tests.fake_engine import OracleFrozenCLIP
    arch = ARCHS["tiny"]
    clip = OracleFrozenCLIP(sd, arch)
    clip._emb = sd["token_embedding.weight"].float()
    clip.tokenizer = default_tokenizer()
    torch.manual_seed(int(case["case_seed"]))
    return PromptLearner(cocoop_cfg(case, arch.image_resolution), [str(n) for n in case["classnames"]], clip)


def test_state_dict_keys_and_shapes_match_reference():
    ref = json.load(open(os.path.join(GOLDEN, "ref_cocoop_prompt_learner.json")))["state_dict"]
    pl = host_prompt_learner(load_npz("tiny_cocoop"), tiny_sd_with_tokens())
    own = {k: list(v.shape) for k, v in pl.state_dict().items()}
    assert list(own) == list(ref), "checkpoint keys (and their order) must be the reference's"
    assert own == ref
    assert all(p.dtype == torch.float32 for p in pl.parameters())                 # fp32 masters


@pytest.mark.parametrize("name", TINY_COCOOP_CASES)
def test_buffers_layout_and_tokens_bit_exact(name):
    case = load_npz(name)
    pl = host_prompt_learner(case, tiny_sd_with_tokens())
    assert np.array_equal(pl.tokenized_prompts.numpy(), case["tokenized_prompts"])
    assert pl.name_lens == case["name_lens"].tolist()
    assert np.array_equal(pl.token_prefix.numpy(), case["token_prefix"])
    assert np.array_equal(pl.token_suffix.numpy(), case["token_suffix"])
    assert np.array_equal(pl.layout.numpy(), case["layout"]), "construct_prompts' layout must be bit-exact"
    assert np.array_equal(pl.eot.numpy().astype(np.int64), case["eot"])
    assert pl.n_ctx == int(case["meta_n_ctx"])


def test_ctx_init_words_give_the_reference_ctx():
    case = load_npz("tiny_cocoop_ctxinit")
    pl = host_prompt_learner(case, tiny_sd_with_tokens())
    n_words = len(str(case["meta_ctx_init"]).replace("_", " ").split(" "))
    assert pl.n_ctx == n_words == int(case["meta_n_ctx"]) != int(case["meta_n_ctx_cfg"])
    assert np.array_equal(pl.ctx.detach().numpy(), case["param_ctx"]), "ctx must start as the words' token embeddings, bit for bit"


def test_random_ctx_init_matches_reference_draw_order():
    """Same seed, same draw order as the reference constructor (ctx, then meta_net): the initial parameters agree."""
    case = load_npz("tiny_cocoop")
    pl = host_prompt_learner(case, tiny_sd_with_tokens())
    assert np.array_equal(pl.ctx.detach().numpy(), case["param_ctx"])
    assert np.array_equal(pl.meta_net.linear1.weight.detach().numpy(), case["param_meta_net.linear1.weight"])


def oracle_cocoop(sd, params, image, label, token_prefix, token_suffix, layout, eot, vision_heads, text_heads):
    """trainers/cocoop.py:171-192 with the CPU oracle's encoders: logits, loss and the gradients of the prompt-learner parameters,
    plus the per-image text features.  meta_net and ctx + bias on torch autograd; the towers' backward is the oracle's."""
    from oracle import clip_oracle as O
    P = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    with torch.no_grad():
        img, _ = O.image_encoder_fwd(sd, image, None, None, heads=vision_heads, need_bwd=False)
    imf = img / img.norm(dim=-1, keepdim=True)
    h = torch.relu(imf @ P["meta_net.linear1.weight"].t() + P["meta_net.linear1.bias"])
    bias = h @ P["meta_net.linear2.weight"].t() + P["meta_net.linear2.bias"]
    ctx_shifted = P["ctx"].unsqueeze(0) + bias.unsqueeze(1)
    scale = float(sd["logit_scale"].float().exp())
    rows, saved, txts = [], [], []
    for g in range(image.shape[0]):
        prompts = O.assemble_prompts(ctx_shifted[g].detach(), token_prefix, token_suffix, layout)
        txt, tctx = O.text_encoder_fwd(sd, prompts, eot, heads=text_heads)
        lg, lctx = O.logits_fwd(img[g:g + 1], txt, scale)
        rows.append(lg)
        saved.append((tctx, lctx))
        txts.append(txt)
    logits = torch.cat(rows)
    loss, dl = O.cross_entropy_fwd_bwd(logits, label)
    dcs = torch.zeros_like(ctx_shifted)
    for g, (tctx, lctx) in enumerate(saved):
        _, dtxt = O.logits_bwd(dl[g:g + 1], lctx)
        dcs[g] = O.scatter_prompt_grad(O.text_encoder_bwd(sd, dtxt, tctx), layout, tuple(ctx_shifted.shape[1:]))
    ctx_shifted.backward(dcs)
    return logits, loss, {k: v.grad for k, v in P.items()}, txts


@pytest.mark.parametrize("name", TINY_COCOOP_CASES)
def test_oracle_reproduces_reference_fixture(name):
    from mvlpt_amd.weights import ARCHS
    case = load_npz(name)
    sd = {k: v for k, v in tiny_sd_with_tokens().items() if k != "token_embedding.weight"}
    arch = ARCHS["tiny"]
    params = {k[len("param_"):]: t(v) for k, v in case.items() if k.startswith("param_")}
    logits, loss, grads, txts = oracle_cocoop(sd, params, t(case["image"]), t(case["label"]), t(case["token_prefix"]),
                                              t(case["token_suffix"]), t(case["layout"]), t(case["eot"]),
                                              arch.vision_heads, arch.transformer_heads)
    tol = 5e-5

    def close(a, b, what):
        err = float((a - t(b)).abs().max()) / max(1.0, float(np.abs(b).max()))
        assert err <= tol, f"{name} {what}: {err:.2e}"
    close(logits.detach(), case["out_logits"], "logits")
    close(loss.detach().reshape(1), case["out_loss"].reshape(1), "loss")
    close(txts[0], case["out_text_features_img0"], "text features of image 0")
    assert set(grads) == {k[len("grad_"):] for k in case if k.startswith("grad_")}
    for k, g in grads.items():
        ref = case["grad_" + k]
        err = float((g - t(ref)).abs().max()) / float(np.abs(ref).max())
        assert err <= tol, f"{name} grad {k}: {err:.2e}"


def test_mvlpt_embedded_cocoop_still_refused():
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import MultitaskVLPromptLearner
    from mvlpt_amd.weights import ARCHS
    from tests.fake_engine import OracleFrozenCLIP
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.TRAINER.MVLPT.COCOOP.N_CTX = 4
    with pytest.raises(NotImplementedError):
        MultitaskVLPromptLearner(cfg, ["a", "b"], OracleFrozenCLIP(tiny_sd_with_tokens(), ARCHS["tiny"]))
    assert get_cfg_default().TRAINER.COCOOP == {"N_CTX": 16, "CTX_INIT": "", "PREC": "fp16"}      # train.py:125-128


# ------------------------------------------------------------------------------------------------ registration order
def _registration_cases():
    """(name, constructor) of one prompt learner per route, on the tiny arch with the hash tokenizer and three classes."""
    from mvlpt_amd.cocoop import PromptLearner
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import MultitaskVLPromptLearner as Base
    from mvlpt_amd.mvlpt_cocoop import MultitaskVLPromptLearner as Route
    from mvlpt_amd.weights import ARCHS
    from tests.fake_engine import OracleFrozenCLIP
    arch = ARCHS["tiny"]
    sd = tiny_sd_with_tokens()
    names = ["cat", "red fox", "aeroplane"]

    def make(cls, coop=0, cocoop=0, vpt=0, deep=False, project=-1):
        def build():
            cfg = get_cfg_default()
            cfg.INPUT.SIZE = (arch.image_resolution, arch.image_resolution)
            T = cfg.TRAINER.MVLPT
            T.COOP.N_CTX, T.COCOOP.N_CTX, T.VPT.N_CTX, T.VPT.DEEP, T.VPT.PROJECT = coop, cocoop, vpt, deep, project
            T.PROJECT_METHOD, T.PROJECT_DIM = "transformer", 64
            cfg.TRAINER.COCOOP.N_CTX = 4
            return cls(cfg, names, OracleFrozenCLIP(sd, arch))
        return build
    return [("coop", make(Base, coop=4)), ("upt_deep_project", make(Base, coop=4, vpt=3, deep=True, project=24)),
            ("cocoop", make(PromptLearner)), ("mvlpt_cocoop_vpt", make(Route, cocoop=4, vpt=3, deep=True, project=24))]


# name: state_dict() keys with shapes, in order.  The order is part of the format of what has been saved so far: the flat prompt
# buffers, the fused optimizer's segments, the broadcast and optimizer checkpoints follow the parameter order, model checkpoints
# the state_dict order.  The three learners share their setup helpers (mvlpt_amd.model), so a change there moves all of them.
_TABLES = [("token_prefix", [3, 1, 128]), ("token_suffix", [3, 72, 128])]
_BUFFERS = _TABLES + [("layout", [3, 77]), ("eot", [3])]
_VPT = [("vpt_embeddings", [1, 3, 24]), ("vpt_embeddings_deep", [2, 3, 24])]
_VPT_PROJ = [("vpt_proj.weight", [128, 24]), ("vpt_proj.bias", [128])]
_META_NET = [("meta_net.linear1.weight", [8, 128]), ("meta_net.linear1.bias", [8]),
             ("meta_net.linear2.weight", [128, 8]), ("meta_net.linear2.bias", [128])]
_MVLPT_PROJ = [("mvlpt_proj.resblocks.0.attn.in_proj_weight", [192, 64]), ("mvlpt_proj.resblocks.0.attn.in_proj_bias", [192]),
               ("mvlpt_proj.resblocks.0.attn.out_proj.weight", [64, 64]), ("mvlpt_proj.resblocks.0.attn.out_proj.bias", [64]),
               ("mvlpt_proj.resblocks.0.ln_1.weight", [64]), ("mvlpt_proj.resblocks.0.ln_1.bias", [64]),
               ("mvlpt_proj.resblocks.0.mlp.c_fc.weight", [256, 64]), ("mvlpt_proj.resblocks.0.mlp.c_fc.bias", [256]),
               ("mvlpt_proj.resblocks.0.mlp.c_proj.weight", [64, 256]), ("mvlpt_proj.resblocks.0.mlp.c_proj.bias", [64]),
               ("mvlpt_proj.resblocks.0.ln_2.weight", [64]), ("mvlpt_proj.resblocks.0.ln_2.bias", [64]),
               ("mvlpt_proj_ctx_vpt_pre.weight", [64, 128]), ("mvlpt_proj_ctx_vpt_pre.bias", [64]),
               ("mvlpt_proj_ctx_vpt_post.weight", [128, 64]), ("mvlpt_proj_ctx_vpt_post.bias", [128]),
               ("mvlpt_proj_ctx_coop_pre.weight", [64, 128]), ("mvlpt_proj_ctx_coop_pre.bias", [64]),
               ("mvlpt_proj_ctx_coop_post.weight", [128, 64]), ("mvlpt_proj_ctx_coop_post.bias", [128])]
# A module's own parameters come first, then (state_dict only) its persistent buffers, then its submodules in registration order;
# named_parameters() is the state_dict without the two buffers, named_buffers() adds the two non-persistent tables.
REGISTRATION = {
    "coop": [("ctx", [4, 128])] + _TABLES,
    "upt_deep_project": _VPT + [("ctx", [4, 128])] + _TABLES + _VPT_PROJ + _MVLPT_PROJ,
    "cocoop": [("ctx", [4, 128])] + _TABLES + _META_NET,
    "mvlpt_cocoop_vpt": _VPT + [("cocoop_ctx", [4, 128])] + _TABLES + _VPT_PROJ + _META_NET,
}


def test_registration_order_of_the_three_prompt_learners():
    cases = _registration_cases()
    assert [n for n, _ in cases] == list(REGISTRATION)
    for name, build in cases:
        torch.manual_seed(11)
        pl = build()
        state = REGISTRATION[name]
        assert [(k, list(v.shape)) for k, v in pl.state_dict().items()] == state, name
        assert [(k, list(v.shape)) for k, v in pl.named_parameters()] == [kv for kv in state if kv not in _TABLES], name
        assert [(k, list(v.shape)) for k, v in pl.named_buffers()] == _BUFFERS, name
