"""Optimizer step on one GPU: microseconds per step of torch.optim against the fused one-launch step (mvlpt_amd.optim) for the
prompt-learner parameter sets of the trainers, and the B = 1 CoCoOp training step with OPTIM.FUSED off and on.  Prints one JSON line.

    python tools/optim_bench.py [--steps 200] [--warmup 20] [--optimizers sgd,adam,adamw] [--no-cocoop]

Parameter sets (ViT-B/16): CoOp-16 (ctx [16, 512]: 1 tensor, 8 192 elements), VPT-deep-8 (2 tensors, 73 728), UPT-4 (the prompt
learner's own tensor list, 566 400) and CoCoOp's ctx + meta_net.  A step is timed as the trainers run it: gradients already in
place, `optimizer.step()` calls back to back on one stream, wall-clock between two device synchronisations (so the host side of the
step — the Python around the launches — counts, as it does at the serial tail of a training step).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def upt4_shapes():
    """The tensors of MultitaskVLPromptLearner under UPT with COOP.N_CTX = VPT.N_CTX = 4, VPT.DEEP, PROJECT_DIM 128 on ViT-B/16
    (text width 512, vision width 768, 12 layers), in named_parameters() order; the projection's shapes come from the module itself."""
    from mvlpt_amd.model import _ProjTransformer
    D, wt, wv, layers, n = 128, 512, 768, 12, 4
    shapes = [(1, n, wv), (layers - 1, n, wv), (n, wt)]
    shapes += [tuple(p.shape) for p in _ProjTransformer(D).parameters()]
    for i, o in ((wv, D), (D, wv), (wt, D), (D, wt)):          # mvlpt_proj_ctx_vpt_pre / _post, mvlpt_proj_ctx_coop_pre / _post
        shapes += [(o, i), (o,)]
    return shapes


def cocoop_shapes(n_ctx=4):
    """CoCoOp's prompt learner on ViT-B/16: ctx [n_ctx, 512], meta_net = Linear(512, 32), Linear(32, 512)."""
    return [(n_ctx, 512), (32, 512), (32,), (512, 32), (512,)]


PARAM_SETS = {
    "coop16": lambda: [(16, 512)],
    "vpt_deep8": lambda: [(1, 8, 768), (11, 8, 768)],
    "upt4": upt4_shapes,
    "cocoop": cocoop_shapes,
}


def numel(shapes):
    return sum(int(torch.Size(s).numel()) for s in shapes)


def make_optimizers(shapes, name, dev, lr=0.002):
    """(torch optimizer, fused optimizer) over two copies of the same parameters with gradients in place."""
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.distributed import FlatGradients, FlatParameters
    from mvlpt_amd.trainer import build_optimizer
    out = []
    for fused in (False, True):
        g = torch.Generator().manual_seed(0)
        mod = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in shapes])
        cfg = get_cfg_default()
        cfg.OPTIM.NAME, cfg.OPTIM.LR, cfg.OPTIM.FUSED = name, lr, fused
        flat = (FlatParameters(mod.parameters()), FlatGradients(mod.parameters())) if fused else None
        opt = build_optimizer(mod, cfg.OPTIM, flat)
        for p in mod.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(dev)
        if fused:
            flat[1].attach()
        out.append(opt)
    return out


def time_steps(opt, warmup, steps):
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def cocoop_step_ms(fused, warmup, steps, classes=100):
    from mvlpt_amd.cocoop import CoCoOp
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import SyntheticDataManager
    from mvlpt_amd.weights import ARCHS
    arch = ARCHS["ViT-B/16"]
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (arch.image_resolution,) * 2
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 1
    cfg.OPTIM.FUSED = fused
    cfg.TRAIN.PRINT_FREQ = 10 ** 9
    cfg.TEST.NO_TEST = True
    dm = SyntheticDataManager(cfg, classes, 1, device="cuda:0")
    tr = CoCoOp(cfg, dm=dm)
    tr.set_model_mode("train")
    tr.num_batches, tr.batch_idx = 10 ** 9, 0
    batch = dm.train_loader_x[0]
    for _ in range(warmup):
        tr.forward_backward(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.forward_backward(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--optimizers", default="sgd,adam,adamw")
    ap.add_argument("--no-cocoop", action="store_true")
    ap.add_argument("--cocoop-steps", type=int, default=30)
    args = ap.parse_args()
    from mvlpt_amd import _lib
    dev = torch.device("cuda:0")
    out = {"metric": "optim_step_us", "library": _lib.lib.mvlpt_version().decode(), "steps": args.steps, "sets": {}}
    for set_name, shapes_fn in PARAM_SETS.items():
        shapes = shapes_fn()
        row = {"tensors": len(shapes), "elements": numel(shapes)}
        for name in args.optimizers.split(","):
            ref, fused = make_optimizers(shapes, name, dev)
            row[name] = {"torch_us": round(time_steps(ref, args.warmup, args.steps), 1),
                         "fused_us": round(time_steps(fused, args.warmup, args.steps), 1)}
        out["sets"][set_name] = row
    if not args.no_cocoop:
        out["cocoop_b1_train_ms"] = {"torch": round(cocoop_step_ms(False, 3, args.cocoop_steps), 3),
                                     "fused": round(cocoop_step_ms(True, 3, args.cocoop_steps), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
