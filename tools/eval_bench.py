"""Times the evaluation routes of MVLPT.test against each other (DESIGN.md scope row f1b), device counters against the host route:

* finalisation of 11point_mAP and roc_auc at (N, C) = (4 952, 20), (32 768, 2), (50 000, 1 000): `evaluator.device_metric` on the
  retained device logits against `metrics.py` on a host copy, the D2H copy of the logits included on the host side;
* 100 multitask CoOp evaluation batches of [100, 2191] logits with 11 tasks: `DeviceClassification.process` + one `evaluate`
  against the per-batch Python loop over `set(tasks_)` (boolean masks, ranged arg-max) that test() ran before.

The two routes of a case run in alternation, `--reps` times each (default 7); the medians are printed, one JSON line per case.
A host run that takes longer than `--slow` seconds is repeated `--slow-reps` times only (the line says how many).
Usage: python tools/eval_bench.py [--reps 7] [--sizes 4952x20,32768x2,50000x1000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvlpt_amd import evaluator as E  # noqa: E402
from mvlpt_amd import metrics as M  # noqa: E402
from mvlpt_amd.config import get_cfg_default  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(device_fn, host_fn, reps, slow, slow_reps):
    dev_ms, host_ms, same = [], [], True
    device_fn()                                                          # warm-up: allocator, first launch
    for r in range(reps):
        ms, got = timed(device_fn)
        dev_ms.append(ms)
        if len(host_ms) < (reps if not host_ms or max(host_ms) < slow * 1e3 else slow_reps):
            ms, want = timed(host_fn)
            host_ms.append(ms)
            same = same and got == want
    return {"device_ms": round(statistics.median(dev_ms), 3), "host_ms": round(statistics.median(host_ms), 3),
            "device_reps": len(dev_ms), "host_reps": len(host_ms), "equal": bool(same)}


def finalisation(N, C, reps, slow, slow_reps):
    g = torch.Generator().manual_seed(N + C)
    logits = torch.randn(N, C, generator=g).to(DEV)
    y = torch.randint(0, C, (N,), generator=g)
    onehot = torch.nn.functional.one_hot(y, C).float().to(DEV)
    for name in ("11point_mAP", "roc_auc"):
        fn = E.device_metric(name)
        res = alternate(lambda: fn(onehot, logits),
                        lambda: M.get_metric(name)(onehot.cpu().numpy(), logits.cpu().numpy()), reps, slow, slow_reps)
        print(json.dumps({"case": "finalisation", "metric": name, "N": N, "C": C, **res}), flush=True)


def parent_loop(batches, ranges):
    """the CoOp branch of MVLPT.test before the device counters"""
    correct, total, per_task = torch.zeros((), device=DEV), 0, {}
    for output, label, tasks_ in batches:
        correct += (output.argmax(dim=1) == label).sum()
        total += label.shape[0]
        for t_id in set(tasks_.tolist()):
            sel = (tasks_ == t_id).to(output.device)
            lo, hi = ranges[t_id]
            hit = (output[sel][:, lo:hi].argmax(dim=1) + lo == label[sel]).sum()
            acc = per_task.setdefault(t_id, [torch.zeros((), device=DEV), 0])
            acc[0] += hit
            acc[1] += int(sel.sum())
    return 100.0 * float(correct) / max(total, 1), {t: 100.0 * float(c) / max(n, 1) for t, (c, n) in per_task.items()}


def coop_batches(reps, slow, slow_reps, n_batches=100, B=100, C=2191, T=11):
    g = torch.Generator().manual_seed(7)
    bounds = np.linspace(0, C, T + 1).astype(int)
    ranges = [(int(bounds[t]), int(bounds[t + 1])) for t in range(T)]
    batches = []
    for _ in range(n_batches):
        tasks_ = torch.randint(0, T, (B,), generator=g)
        lo = torch.tensor([ranges[t][0] for t in tasks_.tolist()])
        width = torch.tensor([ranges[t][1] - ranges[t][0] for t in tasks_.tolist()])
        label = lo + (torch.rand(B, generator=g) * width).long()
        batches.append((torch.randn(B, C, generator=g).to(DEV), label.to(DEV), tasks_))
    cfg = get_cfg_default()

    def device_route():
        ev = E.DeviceClassification(cfg, None, task_ranges=ranges)
        for output, label, tasks_ in batches:
            ev.process(output, label, tasks_)
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            res = ev.evaluate()
        return res["accuracy"], dict(res["task_accuracy"])

    res = alternate(device_route, lambda: parent_loop(batches, ranges), reps, slow, slow_reps)
    print(json.dumps({"case": "coop_multitask_batches", "batches": n_batches, "B": B, "C": C, "tasks": T, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow", type=float, default=5.0)
    ap.add_argument("--slow-reps", type=int, default=1)
    ap.add_argument("--sizes", default="4952x20,32768x2,50000x1000")
    a = ap.parse_args()
    coop_batches(a.reps, a.slow, a.slow_reps)
    for size in a.sizes.split(","):
        N, C = (int(v) for v in size.split("x"))
        finalisation(N, C, a.reps, a.slow, a.slow_reps)


if __name__ == "__main__":
    main()
