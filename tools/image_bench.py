"""Time the image tower forward alone (ViT-B/16, batch 256, no prompts, no backward) through the engine. GPU box only.

  python tools/image_bench.py [ARCH] [B] [--activation quick_gelu|gelu|both] [--reps 7] [--iters 20] [--profile]

ARCH: any ViT name mvlpt_amd.weights.get_arch knows, "ViT-H/14" (16 heads of 80: attention_wide.hip) included.
--profile: one more forward under the engine's profiler: the share of every kernel class in the tower time.

--activation: MODEL.BACKBONE.ACTIVATION (Engine.set_activation).  "both" times the two settings alternately on one engine, rep by rep, and
prints the median of each and their ratio: the price of the stand-alone activation pass (and of the fp32 residual stream it implies)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mvlpt_amd.model import FrozenCLIP
from mvlpt_amd.weights import get_arch, make_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("arch", nargs="?", default="ViT-B/16")
ap.add_argument("B", nargs="?", type=int, default=256)
ap.add_argument("--activation", choices=["quick_gelu", "gelu", "both"], default="quick_gelu")
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
arch = get_arch(args.arch)
B = args.B
kinds = ["quick_gelu", "gelu"] if args.activation == "both" else [args.activation]
eng = FrozenCLIP(make_state_dict(arch, 1), arch=arch).engine      # arch: a state dict does not say the head width ("ViT-H/14": 80)
x = torch.randn(B, 3, arch.image_resolution, arch.image_resolution, device="cuda").half()
for k in kinds:      # warm up every setting that is timed
    eng.set_activation(k)
    for _ in range(3): eng.image_fwd(x)
ms = {k: [] for k in kinds}
for _ in range(args.reps):
    for k in kinds:
        eng.set_activation(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters): eng.image_fwd(x)
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) / args.iters * 1e3)
for k in kinds:
    print(f"image tower fwd {arch.name if hasattr(arch, 'name') else ''} B={B} activation={k}: {statistics.median(ms[k]):.3f} ms "
          f"(min {min(ms[k]):.3f}, max {max(ms[k]):.3f}; median of {args.reps})")
if len(kinds) == 2:
    print(f"   gelu / quick_gelu = {statistics.median(ms['gelu']) / statistics.median(ms['quick_gelu']):.4f}")
if args.profile:
    eng.set_activation(kinds[0])
    eng.profile_begin(True)
    eng.image_fwd(x)
    torch.cuda.synchronize()
    prof = eng.profile_end()
    import re
    classes = {k: v for k, v in prof.items() if not re.match(r"g\d", k)}      # (the per-shape GEMM records repeat the class gemm_bt)
    total = sum(v["ms"] for v in classes.values())
    for name, v in sorted(classes.items(), key=lambda kv: -kv[1]["ms"]):
        if v["launches"]:
            print(f"   {name:22s} {v['launches']:4d} launches {v['ms']:8.3f} ms  {100 * v['ms'] / total:5.1f} %")
