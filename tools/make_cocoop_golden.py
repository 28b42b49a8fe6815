"""TEST INFRASTRUCTURE — generates the CoCoOp fixtures under tests/golden/ from the REAL reference (trainers/cocoop.py).

Run where the reference tree is available (see oracle/ref_shim.py); the GPU tests only read the files it writes:

    python tools/make_cocoop_golden.py

The reference's `trainers.cocoop.CustomCLIP` (trainers/cocoop.py:164-194) is instantiated with PREC = "fp32" on a `clip.model.CLIP`
whose weights come from our deterministic generator (oracle.make_golden.build_ref_clip, used read-only), run on the CPU in eval mode
(logits) and in training mode (F.cross_entropy loss + backward), and inputs / outputs are stored as data:
  tiny_cocoop.npz               tiny arch, N_CTX 4, 5 classes, B 3 (inputs, parameters, buffers, outputs, gradients)
  tiny_cocoop_ctxinit.npz       the same with CTX_INIT "a photo of a"
  full_vitb16_cocoop.npz        ViT-B/16, 10 classes, B 2: parameters and outputs only, images regenerated from `image_seed`
  ref_cocoop_prompt_learner.json  state_dict keys and shapes of the reference PromptLearner
"""
from __future__ import annotations

import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import ARCHS, CLASSNAMES, build_ref_clip  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY_SEED, FULL_SEED = 1, 2          # oracle/make_golden.py: the frozen weights of tiny_clip.npz / the full_* cases


def cocoop_cfg(image_size, n_ctx, ctx_init=""):
    ns = SimpleNamespace
    return ns(TRAINER=ns(COCOOP=ns(N_CTX=n_ctx, CTX_INIT=ctx_init, PREC="fp32")), INPUT=ns(SIZE=(image_size, image_size)))


def layout_from_reference(pl):
    """construct_prompts' row layout, recovered by pushing index markers through the reference (0 = prefix, e > 0 = suffix
    row e - 1, e < 0 = ctx row -e - 1), as oracle/make_golden.layout_from_reference does for forward_coop."""
    C, n, dt = pl.n_cls, pl.n_ctx, pl.token_prefix.shape[-1]
    pre = torch.zeros_like(pl.token_prefix)
    suf = (torch.arange(pl.token_suffix.shape[1]).float() + 1).view(1, -1, 1).expand_as(pl.token_suffix)
    marker = (-(torch.arange(n).float() + 1)).view(1, n, 1).expand(C, n, dt)
    with torch.no_grad():
        out = pl.construct_prompts(marker, pre, suf)
    return out[..., 0].round().to(torch.int32)


def run_cocoop_case(coop, clip_model, *, name, image_size, classnames, B, case_seed, n_ctx, ctx_init="", store_inputs=True):
    cfg = cocoop_cfg(image_size, n_ctx, ctx_init)
    torch.manual_seed(case_seed)
    cc = coop.CustomCLIP(cfg, classnames, clip_model)
    for n_, p in cc.named_parameters():
        p.requires_grad_("prompt_learner" in n_)           # trainers/cocoop.py:220-225
    pl = cc.prompt_learner
    g = torch.Generator().manual_seed(case_seed + 77)
    with torch.no_grad():                                  # non-trivial biases on top of nn.Linear's init
        for n_, p in pl.meta_net.named_parameters():
            if n_.endswith("bias"):
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    C = len(classnames)
    g = torch.Generator().manual_seed(case_seed + 1000)    # inputs have their own stream
    image = torch.randn(B, 3, image_size, image_size, generator=g)
    label = torch.randint(0, C, (B,), generator=g)

    cc.eval()
    with torch.no_grad():
        logits = cc(image)                                 # :193-194
        imf = cc.image_encoder(image)
        imf = imf / imf.norm(dim=-1, keepdim=True)
        prompts = pl(imf)
        txt0 = cc.text_encoder(prompts[0], cc.tokenized_prompts)    # per-image text features of image 0 (unnormalised)
    cc.train()
    loss = cc(image, label)                                # :191-192
    loss.backward()

    d = {
        "meta_n_ctx": np.int64(pl.n_ctx), "meta_n_ctx_cfg": np.int64(n_ctx), "meta_ctx_init": np.array(ctx_init),
        "tokenized_prompts": pl.tokenized_prompts.numpy().astype(np.int64),
        "name_lens": np.array(pl.name_lens, dtype=np.int64),
        "eot": pl.tokenized_prompts.argmax(dim=-1).numpy().astype(np.int64),
        "layout": layout_from_reference(pl).numpy(),
        "label": label.numpy().astype(np.int64),
        "out_logits": logits.numpy(), "out_loss": loss.detach().numpy(),
        "out_text_features_img0": txt0.numpy(),
        "case_seed": np.int64(case_seed), "classnames": np.array(classnames),
    }
    for n_, p in pl.named_parameters():
        d["param_" + n_] = p.detach().numpy()
        d["grad_" + n_] = p.grad.numpy()
    if store_inputs:
        d["image"] = image.numpy()
        d["token_prefix"] = pl.token_prefix.numpy()
        d["token_suffix"] = pl.token_suffix.numpy()
    else:
        d["image_seed"] = np.int64(case_seed + 1000)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(f"[golden] {name}: logits {tuple(logits.shape)} loss {float(loss.detach()):.6f}")
    return pl


def main():
    ref_shim.install()
    cm = importlib.import_module("clip.model")
    coop = importlib.import_module("trainers.cocoop")
    arch = ARCHS["tiny"]
    clip_model, _ = build_ref_clip(cm, arch, TINY_SEED)
    common = dict(image_size=arch.image_resolution, classnames=CLASSNAMES[:5], B=3)
    pl = run_cocoop_case(coop, clip_model, name="tiny_cocoop", case_seed=51, n_ctx=4, **common)
    keys = {k: list(v.shape) for k, v in pl.state_dict().items()}
    with open(os.path.join(OUT, "ref_cocoop_prompt_learner.json"), "w") as f:
        json.dump({"config": "tiny CLIP, COCOOP.N_CTX 4, 5 classes (tests/test_cocoop_host.py)", "state_dict": keys}, f, indent=1)
    run_cocoop_case(coop, clip_model, name="tiny_cocoop_ctxinit", case_seed=52, n_ctx=16, ctx_init="a photo of a", **common)
    arch = ARCHS["ViT-B/16"]
    clip_model, _ = build_ref_clip(cm, arch, FULL_SEED)
    run_cocoop_case(coop, clip_model, name="full_vitb16_cocoop", image_size=224, classnames=CLASSNAMES[:10], B=2, case_seed=53,
                    n_ctx=16, store_inputs=False)


if __name__ == "__main__":
    main()
