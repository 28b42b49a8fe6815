"""TEST INFRASTRUCTURE — generates the ResNet-backbone fixtures under tests/golden/ from the REAL reference.

Run where the reference tree is available (see oracle/ref_shim.py); the tests only read the files it writes:

    python tools/make_resnet_golden.py [features] [trainers] [keys]

A `clip.model.CLIP` with a tuple `vision_layers` (so that its image tower is ModifiedResNet, clip/model.py:94-150, 255-263) is built
on the CPU in fp32 / eval mode, loaded with strict=True from our deterministic generator (mvlpt_amd.weights.make_state_dict on a
ResNetClipArch) and run; only OUTPUTS are stored — weights and images are regenerated from the stored seeds on both sides:
  tiny_rn_features.npz          tiny-rn at B 3, and at resolution 96 / B 2 (a 3 x 3 attention pool: 10 tokens, an odd grid): features
                                and, per stage (stem, layer1..4), mean, rms and a fixed 64-element sample (tests/resnet_ref.summarize)
  full_rn50_features.npz, full_rn101_features.npz      B 2 each, the same contents
  tiny_rn_coop.npz              trainers/coop.py CustomCLIP on tiny-rn: 5 classes, n_ctx 4, logits, loss, grad_ctx
  tiny_rn_cocoop.npz            trainers/cocoop.py (tools/make_cocoop_golden.run_cocoop_case)
  tiny_rn_zsclip.npz            trainers/zsclip.py (tools/make_zsclip_golden.run_case)
  ref_rn50_keys.json            the state_dict keys and shapes of the reference's RN50
"""
from __future__ import annotations

import dataclasses
import importlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import CLASSNAMES, build_ref_clip  # noqa: E402
from mvlpt_amd.weights import RESNET_ARCHS  # noqa: E402
from tests.resnet_ref import STAGES, summarize  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY_SEED, FULL_SEED = 1, 2          # the seeds of the other tiny_* / full_* fixtures


def feature_case(cm, arch, seed, B, image_seed, prefix=""):
    clip_model, _ = build_ref_clip(cm, arch, seed)
    vis = clip_model.visual
    outs = {}
    hooks = [m.register_forward_hook(lambda _m, _i, o, n=n: outs.__setitem__(n, o.detach()))
             for n, m in zip(STAGES, (vis.avgpool, vis.layer1, vis.layer2, vis.layer3, vis.layer4))]
    g = torch.Generator().manual_seed(image_seed)
    image = torch.randn(B, 3, arch.image_resolution, arch.image_resolution, generator=g)
    with torch.no_grad():
        feat = clip_model.encode_image(image)
    for h in hooks:
        h.remove()
    d = {prefix + "features": feat.numpy(), prefix + "weight_seed": np.int64(seed), prefix + "image_seed": np.int64(image_seed),
         prefix + "image_batch": np.int64(B), prefix + "image_resolution": np.int64(arch.image_resolution)}
    for n in STAGES:
        for k, v in summarize(outs[n]).items():
            d[f"{prefix}{n}_{k}"] = v.numpy()
    print(f"[golden] {arch.name} res {arch.image_resolution} B {B}: features {tuple(feat.shape)} max|f| {float(feat.abs().max()):.4f} "
          f"stage rms {[round(float(d[prefix + n + '_rms']), 3) for n in STAGES]}")
    return d


def make_features(cm):
    tiny = RESNET_ARCHS["tiny-rn"]
    d = feature_case(cm, tiny, TINY_SEED, 3, 2001)
    d.update(feature_case(cm, dataclasses.replace(tiny, image_resolution=96), TINY_SEED, 2, 2002, prefix="r96_"))
    np.savez_compressed(os.path.join(OUT, "tiny_rn_features.npz"), **d)
    for name, fix, iseed in (("RN50", "full_rn50_features", 2003), ("RN101", "full_rn101_features", 2004)):
        np.savez_compressed(os.path.join(OUT, fix + ".npz"), **feature_case(cm, RESNET_ARCHS[name], FULL_SEED, 2, iseed))


def make_coop(cm):
    """trainers/coop.py's own PromptLearner / TextEncoder / CustomCLIP, as oracle.make_golden.run_coop_trainer_case drives them."""
    coop = importlib.import_module("trainers.coop")
    arch = RESNET_ARCHS["tiny-rn"]
    clip_model, _ = build_ref_clip(cm, arch, TINY_SEED)
    cfg = ref_shim.make_cfg(input_size=arch.image_resolution, coop_n_ctx=4, class_token_position="end")
    cfg.TRAINER.COOP = cfg.TRAINER.MVLPT.COOP           # trainers/coop.py reads TRAINER.COOP.*
    case_seed, B, names = 71, 3, CLASSNAMES[:5]
    torch.manual_seed(case_seed)
    cc = coop.CustomCLIP(cfg, names, clip_model)
    for n_, p in cc.named_parameters():
        p.requires_grad_("prompt_learner" in n_)
    pl = cc.prompt_learner
    g = torch.Generator().manual_seed(case_seed + 1000)
    image = torch.randn(B, 3, arch.image_resolution, arch.image_resolution, generator=g)
    label = torch.randint(0, len(names), (B,), generator=g)
    logits = cc(image)
    loss = F.cross_entropy(logits, label)
    loss.backward()
    d = {"meta_coop_n_ctx": np.int64(4), "meta_position": np.array("end"), "classnames": np.array(names),
         "tokenized_prompts": pl.tokenized_prompts.numpy().astype(np.int64), "name_lens": np.array(pl.name_lens, dtype=np.int64),
         "token_prefix": pl.token_prefix.detach().numpy(), "token_suffix": pl.token_suffix.detach().numpy(),
         "param_ctx": pl.ctx.detach().numpy(), "grad_ctx": pl.ctx.grad.numpy(), "label": label.numpy().astype(np.int64),
         "image_seed": np.int64(case_seed + 1000), "weight_seed": np.int64(TINY_SEED),
         "out_logits": logits.detach().numpy(), "out_loss": loss.detach().numpy()}
    np.savez_compressed(os.path.join(OUT, "tiny_rn_coop.npz"), **d)
    print(f"[golden] tiny_rn_coop: logits {tuple(logits.shape)} loss {float(loss.detach()):.6f}")


def make_trainers(cm):
    make_coop(cm)
    arch = RESNET_ARCHS["tiny-rn"]
    clip_model, _ = build_ref_clip(cm, arch, TINY_SEED)
    # clip.model.build_model returns model.eval() and the trainers register only the prompt learner with Dassl (trainers/cocoop.py:237),
    # so set_model_mode("train") never reaches the CLIP towers: BatchNorm runs on its running statistics in every step.  The case
    # runner below calls train() on the whole CustomCLIP; pin the image tower to eval as the real training loop leaves it.
    clip_model.visual.train = lambda mode=True: clip_model.visual
    from tools import make_cocoop_golden, make_zsclip_golden
    make_cocoop_golden.run_cocoop_case(importlib.import_module("trainers.cocoop"), clip_model, name="tiny_rn_cocoop",
                                       image_size=arch.image_resolution, classnames=CLASSNAMES[:5], B=3, case_seed=72, n_ctx=4)
    assert not clip_model.visual.training and float(clip_model.visual.bn1.num_batches_tracked) == 0
    names = [c.replace(" ", "_") for c in CLASSNAMES]
    make_zsclip_golden.run_case(importlib.import_module("trainers.zsclip"), importlib.import_module("clip.clip"), clip_model,
                                name="tiny_rn_zsclip", trainer="ZeroshotCLIP", image_size=arch.image_resolution, classnames=names[:5],
                                B=3, case_seed=73)


def make_keys(cm):
    arch = RESNET_ARCHS["RN50"]
    model = cm.CLIP(*arch.ctor_args())
    keys = {k: list(v.shape) for k, v in model.state_dict().items()}
    with open(os.path.join(OUT, "ref_rn50_keys.json"), "w") as f:
        json.dump({"note": "state_dict keys and shapes of clip.model.CLIP built with RN50's constructor arguments (data: names and sizes)",
                   "state_dict": keys}, f, indent=1)
    print(f"[golden] ref_rn50_keys: {len(keys)} tensors")


def main():
    ref_shim.install()
    cm = importlib.import_module("clip.model")
    which = sys.argv[1:] or ["features", "trainers", "keys"]
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if "keys" in which:
        make_keys(cm)
    if "features" in which:
        make_features(cm)
    if "trainers" in which:
        make_trainers(cm)


if __name__ == "__main__":
    main()
