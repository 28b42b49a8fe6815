"""Time the text tower fwd+bwd alone (C=100, L=77, ViT-B/16 text width 512) through the engine. GPU box only.

  python tools/text_bench.py [C] [L] [--act-ckpt N] [--n-ctx 16] [--reps 7] [--iters 20] [--activation quick_gelu|gelu|both]

--act-ckpt N: TRAINER.ACT_CKPT (Engine.set_text_act_ckpt); prints the plan, the workspace bytes of the step and the median over
`reps` timings of `iters` forward + backward pairs each.
--activation: MODEL.BACKBONE.ACTIVATION (Engine.set_activation); "both" times the two settings alternately on one engine, rep by rep."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mvlpt_amd.model import FrozenCLIP, build_prompt_layout
from mvlpt_amd.weights import ARCHS, make_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("C", nargs="?", type=int, default=100)
ap.add_argument("L", nargs="?", type=int, default=77)
ap.add_argument("--act-ckpt", type=int, default=1)
ap.add_argument("--n-ctx", type=int, default=16)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--activation", choices=["quick_gelu", "gelu", "both"], default="quick_gelu")
args = ap.parse_args()

arch = ARCHS["ViT-B/16"]
clip = FrozenCLIP(make_state_dict(arch, 1), precision=os.environ.get("PREC", "split_grad"))
eng = clip.engine
eng.set_text_act_ckpt(args.act_ckpt)
C, L, n = args.C, args.L, args.n_ctx
nl = [1 + (i % 3) for i in range(C)]
layout = build_prompt_layout(nl, n, L, "middle").cuda()
eot = torch.tensor([n + x + 2 for x in nl], dtype=torch.int32).cuda()
pre = torch.randn(C, 1, 512, device="cuda") * 0.02
suf = torch.randn(C, L - 1 - n, 512, device="cuda") * 0.02
ctx = torch.randn(n, 512, device="cuda") * 0.02
dfeat = torch.randn(C, 512, device="cuda") * 1e-3


def run():
    eng.text_fwd(pre, suf, ctx, layout, eot, save_for_bwd=True)
    eng.text_bwd(dfeat)


def runf():
    eng.text_fwd(pre, suf, ctx, layout, eot, save_for_bwd=True)


kinds = ["quick_gelu", "gelu"] if args.activation == "both" else [args.activation]


def timed(fn):
    """{activation: (median, min, max)} over `reps` timings, the settings taken in turn inside every rep"""
    ms = {k: [] for k in kinds}
    for _ in range(args.reps):
        for k in kinds:
            if eng.activation != k:
                run()      # the setting changes only after a completed step (a saving forward alone leaves one open)
                eng.set_activation(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / args.iters * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


ws = {}
for k in kinds:      # warm up every setting that is timed
    eng.set_activation(k)
    for _ in range(3):
        run()
    ws[k] = eng.text_workspace_bytes(C, L, True)
plan = eng.text_act_ckpt_plan()
both, fwd = timed(run), timed(runf)
for k in kinds:
    print(f"text tower C={C} L={L} act_ckpt={args.act_ckpt} activation={k} (segments {[b - a for a, b, _ in plan]}): "
          f"fwd+bwd {both[k][0]:.3f} ms (min {both[k][1]:.3f}, max {both[k][2]:.3f}; median of {args.reps}), "
          f"workspace {ws[k]} bytes ({ws[k] / 2**30:.3f} GiB)")
    print(f"   fwd only {fwd[k][0]:.3f} ms")
if len(kinds) == 2:
    print(f"   gelu / quick_gelu: fwd+bwd {both['gelu'][0] / both['quick_gelu'][0]:.4f}, fwd only {fwd['gelu'][0] / fwd['quick_gelu'][0]:.4f}")
