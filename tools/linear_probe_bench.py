"""Softmax regression of the linear probe: the HIP evaluation (mvlpt_op_softmax_reg_eval) next to the torch formulation on the same
device, and one full fit at C = 1 next to sklearn on the host where sklearn imports.

    python tools/linear_probe_bench.py [--shapes 1600,512,100 16000,512,1000 16000,1024,1000] [--rounds 9] [--sklearn-max-n 1600]

Evaluation: the two routes alternate inside one process (`--rounds` times after a warm-up of each); a time is a device-event interval
around one call, reported as median and minimum, and as fp32 TFLOP/s on the 4 N D K FLOPs of the two products.  The stock route is
`X @ W.T + b`, `log_softmax`, `R.T @ X` in fp32 (loss, gradient of W and b, the three statistics).  Fit: wall time of
SoftmaxRegression(C=1).fit, its iterations and evaluations; `outside_products` is the share of that time not covered by
evaluations x 2 x (the logits product timed through predict, the gradient product has the same FLOPs): row stage, reductions, the
L-BFGS vector algebra and the read-backs.  sklearn runs on at most 16 threads and only up to --sklearn-max-n rows (hours beyond).
Prints one JSON line per shape.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main(argv=None) -> int:
    from mvlpt_amd import engine as E
    from mvlpt_amd.linear_probe import SoftmaxRegression
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1600,512,100", "16000,512,1000", "16000,1024,1000"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sklearn-max-n", type=int, default=1600)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "linear_probe_bench needs a GPU"
    for shape in args.shapes:
        N, D, K = (int(v) for v in shape.split(","))
        rng = np.random.default_rng(0)
        centres = rng.standard_normal((K, D)).astype(np.float32)
        yh = np.arange(N) % K
        # overlapping classes on rows of about unit length, as normalised image features are
        Xh = 0.25 * centres[yh] + rng.standard_normal((N, D)).astype(np.float32)
        Xh /= np.sqrt(D, dtype=np.float32)
        X, y = torch.from_numpy(Xh).cuda(), torch.from_numpy(yh.astype(np.int32)).cuda()
        y64 = y.long()
        theta = (0.05 * torch.randn(K * D + K, generator=torch.Generator().manual_seed(1))).cuda()
        direction = torch.randn_like(theta)
        l2 = 1.0 / N
        ws = E.softmax_reg_workspace(N, D, K, X.device)
        grad, stats = torch.empty_like(theta), torch.empty(4, device=X.device, dtype=torch.float64)

        def fused():
            return E.op_softmax_reg_eval(X, y, theta, l2, dir=direction, grad=grad, stats=stats, ws=ws)

        def stock():
            W, b = theta[:K * D].view(K, D), theta[K * D:]
            logp = torch.log_softmax(X @ W.T + b, dim=1)
            loss = -logp.gather(1, y64[:, None]).mean() + 0.5 * l2 * (W * W).sum()
            R = logp.exp()
            R[torch.arange(N, device=X.device), y64] -= 1.0
            R /= N
            g = torch.cat([(R.T @ X + l2 * W).reshape(-1), R.sum(0)])
            return g, torch.stack([loss, g.abs().max(), g @ direction, g @ g])

        def logits_only():
            return E.op_softmax_reg_predict(X, theta, ws=ws)

        g1, s1 = fused()
        g2, s2 = stock()
        torch.cuda.synchronize()
        diff = float((g1 - g2).abs().max())
        logits_only()
        tf, ts, tl = [], [], []
        for _ in range(args.rounds):
            tf.append(timed(fused)[0])
            ts.append(timed(stock)[0])
            tl.append(timed(logits_only)[0])
        flops = 4.0 * N * D * K
        tera = lambda ms: flops / (ms * 1e-3) / 1e12
        line = {"N": N, "D": D, "K": K, "rounds": args.rounds,
                "eval": {"ms_median": statistics.median(tf), "ms_min": min(tf), "tflops": tera(statistics.median(tf))},
                "stock": {"ms_median": statistics.median(ts), "ms_min": min(ts), "tflops": tera(statistics.median(ts))},
                "logits_product_ms": statistics.median(tl), "max_abs_grad_diff": diff,
                "workspace_bytes": E.softmax_reg_workspace_bytes(N, D, K)}

        trials = []
        clf = SoftmaxRegression(C=1.0, callback=lambda it, ev, t, n, st: trials.append(n))
        clf.fit(Xh, yh)                      # warm-up: allocator, first launches
        trials.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf.fit(Xh, yh)
        torch.cuda.synchronize()
        fit_s = time.perf_counter() - t0
        evals = 1 + sum(trials)
        line["fit"] = {"seconds": fit_s, "n_iter": clf.n_iter_, "evaluations": evals, "status": clf.status_,
                       "outside_products": 1.0 - evals * 2.0 * statistics.median(tl) * 1e-3 / fit_s}
        line["sklearn"] = None
        if N <= args.sklearn_max_n:
            try:
                from sklearn.linear_model import LogisticRegression
                torch.set_num_threads(min(16, os.cpu_count() or 1))
                t0 = time.perf_counter()
                sk = LogisticRegression(solver="lbfgs", max_iter=1000, C=1.0).fit(Xh, yh)
                line["sklearn"] = {"seconds": time.perf_counter() - t0, "n_iter": int(sk.n_iter_[0])}
            except ImportError:
                pass
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
