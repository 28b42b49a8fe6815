"""TEST INFRASTRUCTURE — generates the fixtures of MVLPT's CoCoOp route under tests/golden/ from the REAL reference (trainers/mvlpt.py
with TRAINER.MVLPT.COCOOP.N_CTX != 0).

Run where the reference tree is available (see oracle/ref_shim.py); the tests only read the files it writes:

    python tools/make_mvlpt_cocoop_golden.py

The reference's `trainers.mvlpt.CustomCLIP` (trainers/mvlpt.py:517-583, the branch at :556-581) is instantiated with COCOOP.PREC = "fp32" on
a `clip.model.CLIP` whose weights come from our deterministic generator (oracle.make_golden.build_ref_clip, used read-only) and run on
the CPU: logits = cc(image, task), F.cross_entropy, backward().  Inputs / outputs are stored as data:
  tiny_mvlpt_cocoop.npz             tiny arch, COCOOP.N_CTX 4, 5 classes, B 3, no mask
  tiny_mvlpt_cocoop_mask.npz        per-task mask, task_counts [2, 1, 3], B 6 (tasks repeated and out of order)
  tiny_mvlpt_cocoop_mask_soft.npz   the same with multi-hot soft labels inside the task range
  tiny_mvlpt_cocoop_vpt.npz         + VPT.N_CTX 2, deep (gradients of both visual prompt tensors)
  tiny_mvlpt_cocoop_ctxinit.npz     COCOOP.CTX_INIT "a photo of a"
  tiny_mvlpt_cocoop_cut.npz         TRAINER.CUT_CONTEXTLEN (last of the tiny cases: the reference slices the shared masks in place)
  full_vitb16_mvlpt_cocoop_mask.npz ViT-B/16, 10 classes in 3 tasks, B 3: parameters and outputs only, images from `image_seed`
  ref_mvlpt_cocoop_prompt_learner.json  state_dict keys and shapes of the reference prompt learner (plain and + VPT)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import ARCHS, CLASSNAMES, build_ref_clip  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY_SEED, FULL_SEED = 1, 2          # oracle/make_golden.py: the frozen weights of tiny_clip.npz / the full_* cases


def layout_from_reference(pl):
    """construct_prompts' row layout (0 = prefix, e > 0 = suffix row e - 1, e < 0 = ctx row -e - 1) from index markers."""
    C, n, dt = pl.n_cls, pl.cocoop_n_ctx, pl.token_prefix.shape[-1]
    pre = torch.zeros_like(pl.token_prefix)
    suf = (torch.arange(pl.token_suffix.shape[1]).float() + 1).view(1, -1, 1).expand_as(pl.token_suffix)
    marker = (-(torch.arange(n).float() + 1)).view(1, n, 1).expand(C, n, dt)
    with torch.no_grad():
        out = pl.construct_prompts(marker, pre, suf)
    return out[..., 0].round().to(torch.int32)


def run_case(mv, clip_model, *, name, image_size, classnames, B, case_seed, n_ctx, ctx_init="", task_counts=None, task=None,
             soft_labels=False, store_inputs=True, **cfgkw):
    cfg = ref_shim.make_cfg(input_size=image_size, label_pertask=task_counts is not None, **cfgkw)
    cfg.TRAINER.MVLPT.COCOOP.N_CTX, cfg.TRAINER.MVLPT.COCOOP.CTX_INIT, cfg.TRAINER.MVLPT.COCOOP.PREC = n_ctx, ctx_init, "fp32"
    dm = ref_shim.make_dm(task_counts) if task_counts is not None else None
    torch.manual_seed(case_seed)
    cc = mv.CustomCLIP(cfg, classnames, clip_model, dm=dm)
    for n_, p in cc.named_parameters():
        p.requires_grad_("prompt_learner" in n_)           # trainers/mvlpt.py:855-858
    pl = cc.prompt_learner
    g = torch.Generator().manual_seed(case_seed + 77)
    with torch.no_grad():                                  # non-trivial biases on top of nn.Linear's init
        for n_, p in pl.meta_net.named_parameters():
            if n_.endswith("bias"):
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    C = len(classnames)
    g = torch.Generator().manual_seed(case_seed + 1000)    # inputs have their own stream
    image = torch.randn(B, 3, image_size, image_size, generator=g)
    if task_counts is not None:
        task = torch.tensor(task)
        assert len(task) == B
        starts = np.concatenate([[0], np.cumsum(task_counts)[:-1]])
        label = torch.tensor([int(starts[t_] + torch.randint(0, task_counts[t_], (1,), generator=g)) for t_ in task.tolist()])
        if soft_labels:                                    # multi-hot targets inside the sample's own task range (as tiny_upt_mask_soft)
            hot = torch.zeros(B, C)
            for b, t_ in enumerate(task.tolist()):
                lo, n = int(starts[t_]), int(task_counts[t_])
                hot[b, lo:lo + n] = (torch.rand(n, generator=g) > 0.5).float()
                hot[b, label[b]] = 1.0
            label = hot
    else:
        label = torch.randint(0, C, (B,), generator=g)
    lab = label
    if soft_labels:                                        # trainers/mvlpt.py:914-916
        lab = label.float()
        lab = lab / lab.sum(dim=-1, keepdim=True)
    logits = cc(image, task=task)                          # :540-583
    loss = F.cross_entropy(logits, lab)                    # :931
    loss.backward()

    d = {
        "meta_n_ctx": np.int64(pl.cocoop_n_ctx), "meta_n_ctx_cfg": np.int64(n_ctx), "meta_ctx_init": np.array(ctx_init),
        "meta_vpt_n_ctx": np.int64(pl.vpt_n_ctx),
        "meta_vpt_deep": np.int64(bool(pl.vpt_deep) and pl.vpt_embeddings_deep is not None),
        "meta_cut": np.int64(bool(cfgkw.get("cut_contextlen", False))),
        "tokenized_prompts": pl.tokenized_prompts.numpy().astype(np.int64),
        "name_lens": np.array(pl.name_lens, dtype=np.int64),
        "eot": pl.tokenized_prompts.argmax(dim=-1).numpy().astype(np.int64),
        "layout": layout_from_reference(pl).numpy(),
        "label": label.numpy(),
        "out_logits": logits.detach().numpy(), "out_loss": loss.detach().numpy(),
        "case_seed": np.int64(case_seed), "classnames": np.array(classnames),
    }
    if task is not None:
        d["task"] = task.numpy().astype(np.int64)
        d["task_counts"] = np.array(task_counts, dtype=np.int64)
        d["task_start"] = cc.class_index_pertask_start.numpy().astype(np.int64)
        d["task_end"] = cc.class_index_pertask_end.numpy().astype(np.int64)
    for n_, p in pl.named_parameters():
        d["param_" + n_] = p.detach().numpy()
        d["grad_" + n_] = p.grad.numpy()                   # every parameter of this route has a gradient
    if store_inputs:
        d["image"] = image.numpy()
        d["token_prefix"] = pl.token_prefix.numpy()
        d["token_suffix"] = pl.token_suffix.numpy()
    else:
        d["image_seed"] = np.int64(case_seed + 1000)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(f"[golden] {name}: logits {tuple(logits.shape)} loss {float(loss.detach()):.6f} L {pl.tokenized_prompts.shape[1]}")
    return pl


def main():
    mv, cm = ref_shim.load_reference()
    arch = ARCHS["tiny"]
    clip_model, _ = build_ref_clip(cm, arch, TINY_SEED)
    R = arch.image_resolution
    plain = dict(image_size=R, classnames=CLASSNAMES[:5], B=3)
    mask = dict(image_size=R, classnames=CLASSNAMES[:6], B=6, task_counts=[2, 1, 3], task=[2, 0, 1, 2, 0, 2])
    pl = run_case(mv, clip_model, name="tiny_mvlpt_cocoop", case_seed=61, n_ctx=4, **plain)
    keys = {"plain": {k: list(v.shape) for k, v in pl.state_dict().items()}}
    run_case(mv, clip_model, name="tiny_mvlpt_cocoop_mask", case_seed=62, n_ctx=4, **mask)
    run_case(mv, clip_model, name="tiny_mvlpt_cocoop_mask_soft", case_seed=63, n_ctx=4, soft_labels=True, **mask)
    pl = run_case(mv, clip_model, name="tiny_mvlpt_cocoop_vpt", case_seed=64, n_ctx=4, vpt_n_ctx=2, vpt_deep=True, **mask)
    keys["vpt"] = {k: list(v.shape) for k, v in pl.state_dict().items()}
    with open(os.path.join(OUT, "ref_mvlpt_cocoop_prompt_learner.json"), "w") as f:
        json.dump({"config": "tiny CLIP, TRAINER.MVLPT.COCOOP.N_CTX 4; plain: 5 classes; vpt: 6 classes, VPT.N_CTX 2 deep "
                             "(tests/test_mvlpt_cocoop_host.py)", "state_dict": keys["plain"], "state_dict_vpt": keys["vpt"]}, f, indent=1)
    run_case(mv, clip_model, name="tiny_mvlpt_cocoop_ctxinit", case_seed=65, n_ctx=16, ctx_init="a photo of a", **plain)
    run_case(mv, clip_model, name="tiny_mvlpt_cocoop_cut", case_seed=66, n_ctx=4, cut_contextlen=True, **plain)
    arch = ARCHS["ViT-B/16"]
    clip_model, _ = build_ref_clip(cm, arch, FULL_SEED)
    run_case(mv, clip_model, name="full_vitb16_mvlpt_cocoop_mask", image_size=224, classnames=CLASSNAMES[:10], B=3, case_seed=67,
             n_ctx=16, task_counts=[3, 2, 5], task=[1, 2, 0], store_inputs=False)


if __name__ == "__main__":
    main()
