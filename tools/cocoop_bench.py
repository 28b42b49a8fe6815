"""CoCoOp throughput on one GPU: ms per training step (ViT-B/16, 100 classes, N_CTX 16) at the reference's batch size 1 and at
B = 8, and evaluation images/s at test batch 100.  Prints one JSON line.

    python tools/cocoop_bench.py [--steps 10] [--warmup 3] [--eval-iters 3]

Frozen weights are the synthetic ViT-B/16 of mvlpt_amd.weights (the speed does not depend on their values).  A step is what
CoCoOp.forward_backward does: image tower, meta_net, full-range text tower forward + backward chunk by chunk, optimizer step.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval-iters", type=int, default=3)
    ap.add_argument("--classes", type=int, default=100)
    args = ap.parse_args()

    from mvlpt_amd import _lib
    from mvlpt_amd.cocoop import CustomCLIP
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.trainer import build_optimizer
    from mvlpt_amd.weights import ARCHS, make_state_dict

    dev = torch.device("cuda:0")
    arch = ARCHS["ViT-B/16"]
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (arch.image_resolution,) * 2
    clip = FrozenCLIP(make_state_dict(arch, seed=1), device=dev)
    torch.manual_seed(0)
    model = CustomCLIP(cfg, [f"class {i}" for i in range(args.classes)], clip).to(dev)
    for n, p in model.named_parameters():
        p.requires_grad_("prompt_learner" in n)
    optim = build_optimizer(model.prompt_learner, cfg.OPTIM)
    R = arch.image_resolution
    out = {"metric": "cocoop", "arch": "ViT-B/16", "classes": args.classes, "n_ctx": model.prompt_learner.n_ctx,
           "max_text_workspace_bytes": model.max_text_workspace_bytes, "library": _lib.lib.mvlpt_version().decode()}

    def timed(fn, warmup, iters):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    model.prompt_learner.train()
    for B in (1, 8):
        image = torch.randn(B, 3, R, R, device=dev)
        label = torch.randint(0, args.classes, (B,), device=dev)

        def step():
            optim.zero_grad(set_to_none=False)
            loss = model(image, label)
            loss.backward()
            optim.step()
        out[f"train_ms_b{B}"] = round(timed(step, args.warmup, args.steps), 3)
        out[f"train_chunks_b{B}"] = model.last_chunks
    model.prompt_learner.eval()
    image = torch.randn(100, 3, R, R, device=dev)
    with torch.no_grad():
        ms = timed(lambda: model(image), 1, args.eval_iters)
    out["eval_images_per_s_b100"] = round(100.0 * 1000.0 / ms, 1)
    out["eval_ms_b100"] = round(ms, 2)
    out["eval_chunks_b100"] = model.last_chunks
    out["text_workspace_bytes_per_image_train"] = clip.engine.text_workspace_bytes(args.classes, 77, True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
