"""Times the Tip-Adapter head (mvlpt_op_tip_*) against the published torch formulation on one GPU:

    python tools/tip_bench.py --out profiles/tip_bench.json

Inference logits at N = 256 and 50 000, a fine-tuning step (forward + backward) at B = 256, and the (beta, alpha) search over the
published 200 x 20 grid at N = 10 000 and 50 000, all at NK = 16 000, C = 1 000, D in {512, 1024}.  The baseline is
`exp(-beta (1 - F K^T)) @ one_hot` in torch on the same device, in fp32 and, as the published code runs it, in fp16.  Three alternating
runs of every pair after a warm-up, device events around each timed region; operands are converted to their compute type before the
timed region.  The torch search loop costs the same at every grid point, so its BODY alone is timed over --torch-points grid points and
reported per point, and the products the loop shares (the zero-shot logits and the affinities) are timed once, separately;
`torch_*_ms_total_extrapolated` is shared + per point x grid size and is NOT a measurement.  Every figure goes to one JSON object; nothing here is a pass / fail number.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nk", type=int, default=16000)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--dims", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--infer-rows", type=int, nargs="+", default=[256, 50000])
    ap.add_argument("--search-rows", type=int, nargs="*", default=[10000, 50000])
    ap.add_argument("--train-rows", type=int, default=256)
    ap.add_argument("--grid", type=int, nargs=2, default=[200, 20])
    ap.add_argument("--torch-points", type=int, default=8, help="grid points the torch search loop is timed over")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args(argv)

    import ctypes as C

    import torch

    from mvlpt_amd import _lib
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.tip_adapter import search_grid
    from mvlpt_amd.weights import ARCHS

    if not torch.cuda.is_available():
        raise SystemExit("tip_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda")
    eng = Engine(ARCHS["tiny"], device=dev)
    NK, C_, s, alpha, beta = args.nk, args.classes, 100.0, 1.0, 5.5
    g = torch.Generator(device="cpu").manual_seed(0)

    def unit(x):
        return x / x.norm(dim=-1, keepdim=True)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def alternate(pairs):
        """{name: [ms per run]}: one warm-up of each, then `runs` rounds in the given order."""
        for _, fn in pairs:
            fn()
        torch.cuda.synchronize()
        out = {n: [] for n, _ in pairs}
        for _ in range(args.runs):
            for n, fn in pairs:
                out[n].append(round(timed(fn), 4))
        return out

    results = {"device": torch.cuda.get_device_name(0), "library": _lib.lib.mvlpt_version().decode(), "NK": NK, "C": C_, "rows": []}
    betas, alphas = search_grid((7.0, 3.0), args.grid)
    for D in args.dims:
        key_cls = torch.arange(NK) * C_ // NK                                    # sorted, NK / C keys per class
        key_ptr = torch.searchsorted(key_cls, torch.arange(C_ + 1)).to(torch.int32).to(dev)
        K = unit(torch.randn(NK, D, generator=g)).to(dev)
        W = unit(torch.randn(C_, D, generator=g)).to(dev)
        one_hot = {torch.float32: torch.nn.functional.one_hot(key_cls, C_).float().to(dev)}
        one_hot[torch.float16] = one_hot[torch.float32].half()

        Kt, Wt = {torch.float32: K, torch.float16: K.half()}, {torch.float32: W, torch.float16: W.half()}      # converted once, untimed

        def torch_logits(Fh, be, al, dt):
            return s * Fh @ Wt[dt].t() + ((-1) * (be - be * (Fh @ Kt[dt].t()))).exp() @ one_hot[dt] * al

        for N in args.infer_rows:
            F = unit(torch.randn(N, D, generator=g)).to(dev)
            F16 = F.half()
            t = alternate([("hip", lambda: eng.tip_logits(F, K, key_ptr, W, s, alpha, beta)),
                           ("torch_fp32", lambda: torch_logits(F, beta, alpha, torch.float32)),
                           ("torch_fp16", lambda: torch_logits(F16, beta, alpha, torch.float16))])
            results["rows"].append({"what": "logits", "N": N, "D": D, "ms": t})
            print(json.dumps(results["rows"][-1]), flush=True)

        B = args.train_rows
        F = unit(torch.randn(B, D, generator=g)).to(dev)
        y = torch.randint(0, C_, (B,), generator=g).to(dev)
        y32 = y.to(torch.int32)

        def hip_step():
            eng.tip_train_fwd(F, y32, K, key_ptr, W, s, alpha, beta)
            eng.tip_train_bwd()

        Ft = {torch.float32: F, torch.float16: F.half()}
        Kp = {dt: Kt[dt].clone().requires_grad_(True) for dt in Kt}      # the published adapter holds its keys in the compute type

        def torch_step(dt):
            Kp[dt].grad = None
            z = s * Ft[dt] @ Wt[dt].t() + ((-1) * (beta - beta * (Ft[dt] @ Kp[dt].t()))).exp() @ one_hot[dt] * alpha
            torch.nn.functional.cross_entropy(z.float(), y).backward()

        t = alternate([("hip", hip_step), ("torch_fp32", lambda: torch_step(torch.float32)), ("torch_fp16", lambda: torch_step(torch.float16))])
        need = C.c_int64()
        _lib.check(_lib.lib.mvlpt_tip_workspace_bytes(B, NK, C_, D, 0, 0, _lib.TIP_TRAIN, C.byref(need)), None, "tip_workspace_bytes")
        results["rows"].append({"what": "train_step", "N": B, "D": D, "ms": t, "workspace_bytes": need.value})
        print(json.dumps(results["rows"][-1]), flush=True)

        for N in args.search_rows:
            F = unit(torch.randn(N, D, generator=g)).to(dev)
            y = torch.randint(0, C_, (N,), generator=g).to(dev)
            y32 = y.to(torch.int32)
            bt, at = torch.tensor(betas, device=dev), torch.tensor(alphas, device=dev)
            pts = [(betas[(i * 37) % len(betas)], alphas[(i * 7) % len(alphas)]) for i in range(args.torch_points)]

            def shared(dt):
                Fh = F.to(dt)
                return s * Fh @ Wt[dt].t(), Fh @ Kt[dt].t()

            held = {dt: shared(dt) for dt in Kt}             # the loop's inputs, formed once and untimed

            def torch_points(dt):
                clip, affinity = held[dt]
                for be, al in pts:                                               # the body of the published double loop, alone
                    z = clip + ((-1) * (be - be * affinity)).exp() @ one_hot[dt] * al
                    (z.argmax(1) == y).sum()

            t = alternate([("hip", lambda: eng.tip_search(F, y32, K, key_ptr, W, s, bt, at)),
                           ("torch_fp32_points", lambda: torch_points(torch.float32)),
                           ("torch_fp16_points", lambda: torch_points(torch.float16)),
                           ("torch_fp32_shared", lambda: shared(torch.float32)),
                           ("torch_fp16_shared", lambda: shared(torch.float16))])
            n_grid = len(betas) * len(alphas)
            _lib.check(_lib.lib.mvlpt_tip_workspace_bytes(N, NK, C_, D, len(betas), len(alphas), _lib.TIP_SEARCH, C.byref(need)), None,
                       "tip_workspace_bytes")
            row = {"what": "search", "N": N, "D": D, "grid": [len(betas), len(alphas)], "ms": t, "torch_points": len(pts),
                   "workspace_bytes": need.value}
            for k in ("torch_fp32", "torch_fp16"):
                per = min(t[k + "_points"]) / len(pts)      # the loop body alone; the shared products are counted once below
                row[k + "_ms_per_point"] = round(per, 4)
                row[k + "_ms_total_extrapolated"] = round(min(t[k + "_shared"]) + per * n_grid, 1)
            del held
            results["rows"].append(row)
            print(json.dumps(row), flush=True)
            del F
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
