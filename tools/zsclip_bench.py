"""Zero-shot CLIP with prompt ensembling on one GPU: the 80 x 1000 ImageNet prompt set (ViT-B/16) through `FrozenCLIP.encode_text` plus
`mvlpt_text_ensemble`, trimmed and bucketed against every chunk forced to the full context length, and the evaluation rate of
`model_inference` at batch 100.  Prints one JSON line.

    python tools/zsclip_bench.py [--repeats 2] [--templates tests/golden/zsclip_templates.json] [--classes 1000]

The prompts are the shipped ImageNet class list (mvlpt_amd.class_prompts) in the template file's 80 ImageNet templates (templates are
data, not package content: INTEGRATION.md §4d).  Both variants run in the same process on the same library, alternating; a time is a
host clock around encode_text + ensemble ending in a device synchronise (host planning and the id uploads are part of what a user
waits for).  Frozen weights are the synthetic ViT-B/16 of mvlpt_amd.weights (the speed does not depend on their values).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--eval-iters", type=int, default=5)
    ap.add_argument("--templates", default=os.path.join(ROOT, "tests", "golden", "zsclip_templates.json"))
    args = ap.parse_args()

    from mvlpt_amd import _lib
    from mvlpt_amd.class_prompts import class_names
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    from mvlpt_amd.zsclip import build_prompts

    with open(args.templates) as f:
        templates = json.load(f)["imagenet"]
    names = [n.rstrip(" .") for n in class_names("imagenet1k")][:args.classes]
    T, C = len(templates), len(names)
    dev = torch.device("cuda:0")
    arch = ARCHS["ViT-B/16"]
    clip = FrozenCLIP(make_state_dict(arch, seed=1, include_token_embedding=True), device=dev)
    t0 = time.perf_counter()
    ids = clip.tokenizer.tokenize(build_prompts(templates, names), clip.context_length)
    tokenize_s = time.perf_counter() - t0
    S = ids.shape[0]
    out = {"metric": "zsclip_encode", "arch": "ViT-B/16", "templates": T, "classes": C, "sequences": S,
           "tokenize_s": round(tokenize_s, 2), "max_text_workspace_bytes": clip.max_text_workspace_bytes,
           "library": _lib.lib.mvlpt_version().decode(), "timer": "host perf_counter around work ending in a device synchronise"}

    def run(trim):
        torch.cuda.synchronize()
        a = time.perf_counter()
        txt = clip.engine.text_ensemble(clip.encode_text(ids, trim=trim).view(T, C, -1))
        torch.cuda.synchronize()
        return time.perf_counter() - a, txt, list(clip.last_text_chunks)

    results = {True: [], False: []}
    feats = {}
    for trim in (True, False):                  # warm-up: workspace growth, code objects, the token-embedding upload
        _, feats[trim], chunks = run(trim)
        out["chunks_trimmed" if trim else "chunks_full"] = chunks
        out["positions_trimmed" if trim else "positions_full"] = sum(L * n for L, n in chunks)
    from bench import _ClockSampler             # engine clock and board power from the amdgpu hwmon files while the timed runs go
    clk = _ClockSampler()
    clk.start()
    for _ in range(args.repeats):               # alternating
        for trim in (True, False):
            results[trim].append(round(run(trim)[0], 4))
    out["clock"] = clk.stop()
    out["encode_s_trimmed"], out["encode_s_full"] = results[True], results[False]
    out["position_ratio"] = round(out["positions_trimmed"] / float(77 * S), 4)
    out["time_ratio"] = round(min(results[True]) / min(results[False]), 4)
    out["max_abs_diff_trimmed_vs_full"] = float((feats[True] - feats[False]).abs().max())

    R = arch.image_resolution
    image = torch.randn(100, 3, R, R, device=dev)
    scale = float(clip.logit_scale.exp())

    def infer():
        return clip.engine.logits_fwd(clip.encode_image(image), feats[True], scale)

    infer()
    torch.cuda.synchronize()
    a = time.perf_counter()
    for _ in range(args.eval_iters):
        infer()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - a) * 1000.0 / args.eval_iters
    out["eval_ms_b100"] = round(ms, 2)
    out["eval_images_per_s_b100"] = round(100.0 * 1000.0 / ms, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
