"""MVLPT's CoCoOp route on one GPU, ranged against dense: ViT-B/16, the `elevater20` class tables (20 tasks, 1151 classes),
COCOOP.N_CTX 16, per-task mask.  Prints one JSON line.

    python tools/mvlpt_cocoop_bench.py [--steps 5] [--warmup 2] [--batch 32] [--dense-batch 4] [--eval-batch 100] [--dense-eval-batch 8]

Tasks are drawn with a fixed seed (a) in proportion to their class counts (k-shot sampling) and (b) evenly.  Per draw: training ms per
step (forward, cross-entropy, backward, optimizer step) and evaluation images/s, each for the ranged text tower and for the dense
tower (every range full), with sequences per step, chunks and text workspace bytes.  Dense at the config's batch 32 is 36 832 sequences per step
(dozens of chunks under the default budget), so dense is timed at `--dense-batch` / `--dense-eval-batch` images and the line says so;
`*_ms_per_kseq` (ms per 1000 text sequences) is the figure to compare: the step's text time should follow the sequence count.
Ranged and dense alternate in one process; every figure is event-timed after warm-up.
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dense-batch", type=int, default=4)
    ap.add_argument("--eval-batch", type=int, default=100)
    ap.add_argument("--dense-eval-batch", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from mvlpt_amd import _lib
    from mvlpt_amd.class_prompts import MultitaskBook, load_class_prompts
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.mvlpt_cocoop import CustomCLIP
    from mvlpt_amd.trainer import build_optimizer
    from mvlpt_amd.weights import ARCHS, make_state_dict

    dev = torch.device("cuda:0")
    arch = ARCHS["ViT-B/16"]
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (arch.image_resolution,) * 2
    cfg.TRAINER.MVLPT.COCOOP.N_CTX = 16
    cfg.DATASET.MULTITASK = cfg.DATASET.MULTITASK_LABEL_PERTASK = True
    book = MultitaskBook.from_list("elevater20")
    counts = torch.tensor(book.num_classes_list)
    starts = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)[:-1]])
    clip = FrozenCLIP(make_state_dict(arch, seed=1), device=dev)
    torch.manual_seed(args.seed)
    model = CustomCLIP(cfg, book.classnames, clip, dm=book, pretokenized=load_class_prompts("elevater20", 16)[0]).to(dev)
    for n, p in model.named_parameters():
        p.requires_grad_("prompt_learner" in n)
    optim = build_optimizer(model.prompt_learner, cfg.OPTIM)
    pl = model.prompt_learner
    R, L = arch.image_resolution, pl.layout.shape[1]
    out = {"metric": "mvlpt_cocoop", "arch": "ViT-B/16", "classes": pl.n_cls, "tasks": len(counts), "n_ctx": pl.cocoop_n_ctx,
           "max_text_workspace_bytes": model.max_text_workspace_bytes, "library": _lib.lib.mvlpt_version().decode(),
           "note": f"ranged at batch {args.batch} / eval {args.eval_batch}; dense at batch {args.dense_batch} / eval "
                   f"{args.dense_eval_batch} (dense at batch 32 is 36832 sequences per step)"}

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

    gen = torch.Generator().manual_seed(args.seed)
    for draw, weights in (("kshot", counts.float()), ("even", torch.ones(len(counts)))):
        nmax = max(args.batch, args.eval_batch)
        task_all = torch.multinomial(weights, nmax, replacement=True, generator=gen)
        label_all = starts[task_all] + (torch.rand(nmax, generator=gen) * counts[task_all]).long()
        image_all = torch.randn(nmax, 3, R, R, device=dev)
        for ranged, B, Be in ((True, args.batch, args.eval_batch), (False, args.dense_batch, args.dense_eval_batch)) * 2:
            tag = f"{draw}_{'ranged' if ranged else 'dense'}"
            model.ranged_text = ranged
            image, task, label = image_all[:B], task_all[:B], label_all[:B].to(dev)

            def step():
                optim.zero_grad(set_to_none=False)
                loss = model.cross_entropy(model(image, task=task), label)
                loss.backward()
                optim.step()
            pl.train()
            ms = timed(step, args.warmup, args.steps)
            seq = model.last_sequences
            out[tag + "_train"] = {"batch": B, "ms": round(ms, 2), "sequences": seq, "chunks": model.last_chunks,
                                   "recompute": bool(model.last_recompute), "ms_per_kseq": round(1000.0 * ms / seq, 2),
                                   "text_workspace_bytes": clip.engine.text_workspace_bytes(
                                       max(c[2] for c in model.chunks(*_ranges(model, task, B, ranged), L, True)), L, True)}
            pl.eval()
            ie, te = image_all[:Be], task_all[:Be]
            with torch.no_grad():
                ms = timed(lambda: model(ie, task=te), 1, max(1, args.steps // 2))
            out[tag + "_eval"] = {"batch": Be, "ms": round(ms, 2), "images_per_s": round(Be * 1000.0 / ms, 1),
                                  "sequences": model.last_sequences, "chunks": model.last_chunks,
                                  "ms_per_kseq": round(1000.0 * ms / model.last_sequences, 2)}
        r, d = out[f"{draw}_ranged_train"], out[f"{draw}_dense_train"]
        out[f"{draw}_sequences_per_image_ranged"] = round(r["sequences"] / r["batch"], 1)
        out[f"{draw}_train_ms_per_kseq_ranged_over_dense"] = round(r["ms_per_kseq"] / d["ms_per_kseq"], 3)
    print(json.dumps(out))


def _ranges(model, task, B, ranged):
    from mvlpt_amd.per_image_text import class_ranges
    n = model.prompt_learner.n_cls
    if not ranged:
        return [0] * B, [n] * B
    return class_ranges(task, model.class_index_pertask_start, model.class_index_pertask_end, B, n)


if __name__ == "__main__":
    main()
