"""Nearest vocabulary tokens: the fused HIP kernel (mvlpt_op_nearest_rows) next to torch.cdist + torch.topk on the same device.

    python tools/interpret_bench.py [--rows 16 1600 16000] [--rounds 7]

Real-size table (V 49408, d 512), k 5, seeded N(0, 0.02) data on both sides.  Per case the two routes alternate inside one process
(`--rounds` times after a warm-up of each); a time is a device-event interval around one call, reported as median and minimum.
Peak memory is torch's allocator peak above the inputs during one call: for the fused route the partial lists and the outputs, for
the stock route the [R, V] distance matrix and what cdist / topk allocate beside it.  Prints one JSON line per case; a case whose
stock route does not fit is reported with "stock": null.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V, D, K = 49408, 512, 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def main(argv=None) -> int:
    from mvlpt_amd.engine import nearest_workspace_bytes, op_nearest_rows
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 1600, 16000])
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "interpret_bench needs a GPU"
    g = torch.Generator().manual_seed(0)
    table = (0.02 * torch.randn(V, D, generator=g)).cuda()
    for R in args.rows:
        q = (0.02 * torch.randn(R, D, generator=g)).cuda()

        def fused():
            return op_nearest_rows(q, table, K)

        def stock():
            dist, idx = torch.topk(torch.cdist(q, table), K, dim=1, largest=False)
            return idx, dist

        fused_peak, (fi, fd) = peak_of(fused)
        try:
            stock_peak, (si, sd) = peak_of(stock)
        except torch.OutOfMemoryError:
            stock_peak = None
        tf, ts = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused)[0])
            if stock_peak is not None:
                ts.append(timed(stock)[0])
        line = {"R": R, "V": V, "d": D, "k": K, "rounds": args.rounds,
                "fused": {"ms_median": statistics.median(tf), "ms_min": min(tf), "peak_bytes": fused_peak,
                          "workspace_bytes": nearest_workspace_bytes(R, V, D, K)},
                "stock": None}
        if stock_peak is not None:
            agree = float((fi.long() == si).float().mean())      # cdist may use the expanded form: near-ties can swap
            line["stock"] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "peak_bytes": stock_peak,
                             "index_agreement": agree, "max_abs_dist_diff": float((fd - sd).abs().max())}
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
