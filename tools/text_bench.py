"""Time the text tower fwd+bwd alone (C=100, L=77, ViT-B/16 text width 512) through the engine. GPU box only.

  python tools/text_bench.py [C] [L] [--act-ckpt N] [--n-ctx 16] [--reps 7] [--iters 20] [--activation quick_gelu|gelu|both]
                             [--deep N [N ...]] [--profile]

--act-ckpt N: TRAINER.ACT_CKPT (Engine.set_text_act_ckpt); prints the plan, the workspace bytes of the step and the median over
`reps` timings of `iters` forward + backward pairs each.
--activation: MODEL.BACKBONE.ACTIVATION (Engine.set_activation); "both" times the two settings alternately on one engine, rep by rep.
--deep N: TRAINER.MVLPT.COOP.N_DEEP, deep text prompts in front of blocks 1 .. N (Engine.text_fwd_deep / text_bwd_deep; 0: the plain
entries).  Several values are timed alternately on one engine, rep by rep, and the extra time over the first is printed.
--profile: one profiled step per --deep value behind the timings: milliseconds and launches per kernel class (the glue class holds the
overwrites and the gathers; every ln_1 that is no longer folded shows as one more layernorm_fwd launch)."""
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
ap.add_argument("--deep", type=int, nargs="+", default=[0])
ap.add_argument("--profile", action="store_true")
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
if any(d < 0 or d > arch.transformer_layers - 1 for d in args.deep):
    ap.error(f"--deep must lie in [0, {arch.transformer_layers - 1}]")
deep_rows = {d: (torch.randn(d, n, 512, device="cuda") * 0.02 if d else None) for d in args.deep}
deep = args.deep[0]      # the setting run() / runf() time


def run():
    if deep:
        eng.text_fwd_deep(pre, suf, ctx, deep_rows[deep], layout, eot, save_for_bwd=True)
        eng.text_bwd_deep(dfeat)
    else:
        eng.text_fwd(pre, suf, ctx, layout, eot, save_for_bwd=True)
        eng.text_bwd(dfeat)


def runf():
    if deep:
        eng.text_fwd_deep(pre, suf, ctx, deep_rows[deep], layout, eot, save_for_bwd=True)
    else:
        eng.text_fwd(pre, suf, ctx, layout, eot, save_for_bwd=True)


acts = ["quick_gelu", "gelu"] if args.activation == "both" else [args.activation]
kinds = [(a, d) for a in acts for d in args.deep]


def timed(fn):
    """{(activation, deep): (median, min, max)} over `reps` timings, the settings taken in turn inside every rep"""
    global deep
    ms = {k: [] for k in kinds}
    for _ in range(args.reps):
        for k in kinds:
            if eng.activation != k[0]:
                run()      # the setting changes only after a completed step (a saving forward alone leaves one open)
                eng.set_activation(k[0])
            deep = k[1]
            run()          # one untimed step of this setting
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / args.iters * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


ws = {}
for k in kinds:      # warm up every setting that is timed
    if eng.activation != k[0]:
        eng.set_activation(k[0])
    deep = k[1]
    for _ in range(3):
        run()
    ws[k] = eng.text_workspace_bytes(C, L, True)      # (deep prompts reserve nothing more: the same figure)
plan = eng.text_act_ckpt_plan()
both, fwd = timed(run), timed(runf)
for k in kinds:
    print(f"text tower C={C} L={L} act_ckpt={args.act_ckpt} activation={k[0]} deep={k[1]} (segments {[b - a for a, b, _ in plan]}): "
          f"fwd+bwd {both[k][0]:.3f} ms (min {both[k][1]:.3f}, max {both[k][2]:.3f}; median of {args.reps}), "
          f"workspace {ws[k]} bytes ({ws[k] / 2**30:.3f} GiB)")
    print(f"   fwd only {fwd[k][0]:.3f} ms")
if len(acts) == 2:
    for d in args.deep:
        g, q = both[("gelu", d)][0], both[("quick_gelu", d)][0]
        print(f"   deep={d} gelu / quick_gelu: fwd+bwd {g / q:.4f}, fwd only {fwd[('gelu', d)][0] / fwd[('quick_gelu', d)][0]:.4f}")
for a in acts:
    for d in args.deep[1:]:
        b0, b1 = both[(a, args.deep[0])][0], both[(a, d)][0]
        f0, f1 = fwd[(a, args.deep[0])][0], fwd[(a, d)][0]
        print(f"   {a} deep={d} over deep={args.deep[0]}: fwd+bwd {b1 - b0:+.3f} ms ({b1 / b0:.4f}), fwd only {f1 - f0:+.3f} ms ({f1 / f0:.4f})")
if args.profile:
    for k in kinds:
        if eng.activation != k[0]:
            run()
            eng.set_activation(k[0])
        deep = k[1]
        run()
        torch.cuda.synchronize()
        eng.profile_begin(True)
        run()
        torch.cuda.synchronize()
        stats = eng.profile_end()
        print(f"profile activation={k[0]} deep={k[1]}: " + "; ".join(
            f"{name} {v['ms']:.3f} ms / {v['launches']} launches" for name, v in sorted(stats.items()) if v.get("launches")))
