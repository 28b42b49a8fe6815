"""Test-time prompt tuning on one GPU: ms per test image of one tuning step plus the final classification (ViT-B/16, V = 64 views,
k = 6, n_ctx 4, CUT_CONTEXTLEN) at C = 100 and C = 1000 classes and G = 1, 4, 16 images tuned side by side, with the chunk counts.
Prints one JSON line (and writes it to --out).

    python tools/tpt_bench.py [--runs 7] [--classes 100 1000] [--groups 1 4 16] [--out profiles/tpt_bench.json]

Two variants run on the SAME engine towers, alternating run by run: "fused", the head of csrc/tpt.hip (mvlpt_op_tpt_head_fwd / _bwd),
and "stock", the same loop with the head written in torch ops (matmul, log_softmax, topk, logsumexp, autograd for dtxt).  The stock
formulation is the comparator, not a G = 1 run of the fused code.  Per configuration: the median over --runs (at least 7) alternating
runs, with the minimum and the maximum.  The view features are computed once outside the timed region for both variants (the image
tower is the same call either way); `image_ms` reports it separately.  Frozen weights are the synthetic ViT-B/16 of mvlpt_amd.weights.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, K = 64, 6


def stock_head(img, txt, scale, k):
    """(loss [G], dtxt [G*C, e]) from torch ops; the selection is constant for the gradient, as in the published method."""
    G, Vn, e = img.shape
    t = txt.detach().requires_grad_(True)
    with torch.enable_grad():
        imn = img / img.norm(dim=-1, keepdim=True)
        tn = (t / t.norm(dim=-1, keepdim=True)).view(G, -1, e)
        z = scale * torch.matmul(imn, tn.transpose(1, 2))
        logp = torch.log_softmax(z, dim=-1)
        H = -(logp.exp() * logp).sum(-1)
        sel = torch.topk(H.detach(), k, dim=-1, largest=False).indices
        lps = torch.gather(logp, 1, sel.unsqueeze(-1).expand(G, k, logp.shape[-1]))
        a = torch.logsumexp(lps, dim=1) - math.log(k)
        loss = -(a.exp() * a).sum(-1)
        (dtxt,) = torch.autograd.grad(loss.sum(), t)
    return loss.detach(), dtxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--classes", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.runs < 7:
        raise SystemExit("--runs must be at least 7 (median of alternating runs)")

    from mvlpt_amd import _lib
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.tpt import CustomCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict

    dev = torch.device("cuda:0")
    arch = ARCHS["ViT-B/16"]
    clip = FrozenCLIP(make_state_dict(arch, seed=1, include_token_embedding=True), device=dev)
    R = arch.image_resolution
    out = {"metric": "tpt", "arch": "ViT-B/16", "views": V, "k": K, "n_ctx": 4, "cut_contextlen": True, "steps": 1, "runs": args.runs,
           "library": _lib.lib.mvlpt_version().decode(), "configs": []}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for C in args.classes:
        cfg = get_cfg_default()
        cfg.INPUT.SIZE = (R, R)
        cfg.TRAINER.CUT_CONTEXTLEN = True
        cfg.TRAINER.TPT.N_VIEWS, cfg.TRAINER.TPT.SELECTION_P = V, 0.1
        torch.manual_seed(0)
        model = CustomCLIP(cfg, [f"class {i}" for i in range(C)], clip).to(dev)
        assert model.k == K
        eng, pl = model.engine, model.prompt_learner
        for G in args.groups:
            views = torch.randn(G * V, 3, R, R, device=dev)
            image_ms = timed(lambda: eng.image_fwd(views, None, None, save_for_bwd=False))
            feats = eng.image_fwd(views, None, None, save_for_bwd=False).view(G, V, -1)
            del views

            def run(fused: bool):
                """one tuning step + the final classification, from given view features"""
                ctx0 = pl.ctx.detach()
                ctx = ctx0.unsqueeze(0).expand(G, *ctx0.shape).clone()
                holder, optim = model._optimizer(ctx)
                if fused:
                    _, _, _, dctx = model.tune_step(feats, holder.ctx.data)
                else:
                    lo, hi = model.full_ranges(G)
                    chunks = model.chunks(lo, hi, model.text_len(ctx), save_for_bwd=True)
                    dctx = torch.empty_like(ctx)
                    for g0, g1, _ in chunks:
                        txt = model.text_chunk(holder.ctx.data, lo, hi, g0, g1, save=True)
                        _, dtxt = stock_head(feats[g0:g1], txt, model.logit_scale_exp, K)
                        dctx[g0:g1] = eng.text_bwd(dtxt)
                    model.last_chunks = len(chunks)
                holder.ctx.grad = dctx
                optim.step()
                tuning_chunks = model.last_chunks
                model.ranged_logits(feats[:, 0].contiguous(), holder.ctx.data, *model.full_ranges(G))
                model.last_chunks = tuning_chunks            # the row reports the tuning step's chunk count

            with torch.no_grad():
                for fused in (True, False):              # warm-up: workspaces, allocator
                    run(fused)
                chunks = model.last_chunks
                ms = {True: [], False: []}
                for _ in range(args.runs):               # alternating
                    for fused in (True, False):
                        ms[fused].append(timed(lambda: run(fused)))
            row = {"classes": C, "images": G, "chunks": chunks, "text_len": int(pl.layout.shape[1]), "image_ms": round(image_ms, 3)}
            for name, key in (("fused", True), ("stock", False)):
                per = [t / G for t in ms[key]]
                row[name] = {"ms_per_image_median": round(statistics.median(per), 3), "min": round(min(per), 3), "max": round(max(per), 3)}
            # the head alone (forward + backward on given features), the same alternation
            txt = torch.randn(G * C, feats.shape[-1], device=dev) * 0.02
            heads = {"fused": lambda: (eng.tpt_head_fwd(feats, txt, model.logit_scale_exp, K), eng.tpt_head_bwd()),
                     "stock": lambda: stock_head(feats, txt, model.logit_scale_exp, K)}
            hms = {n: [] for n in heads}
            for n, fn in heads.items():
                fn()
            for _ in range(args.runs):
                for n, fn in heads.items():
                    hms[n].append(timed(fn))
            for n in heads:
                row[n]["head_ms_median"] = round(statistics.median(hms[n]), 4)
                row[n]["head_ms_min"], row[n]["head_ms_max"] = round(min(hms[n]), 4), round(max(hms[n]), 4)
            out["configs"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
