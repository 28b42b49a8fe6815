"""Linear-probe CLIP baseline with the fits on the device.  Takes the arguments of the reference's lpclip/linear_probe.py and writes
its two report files (`report/{feature_dir}_s{num_step}r{num_run}[_details].txt`, appended, same line formats):

    python tools/linear_probe.py --dataset Caltech101 --num_step 8 --num_run 10 --feature_dir clip_feat

reads `{feature_dir}/{dataset}/{train,val,test}.npz` (keys feature_list / label_list), the files the reference's
lpclip/feat_extractor.py writes and mvlpt_amd.linear_probe.save_split writes from this engine's towers: they cross both ways.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", type=str, default="", help="path to dataset")
    ap.add_argument("--num_step", type=int, default=8, help="number of steps")
    ap.add_argument("--num_run", type=int, default=10, help="number of runs")
    ap.add_argument("--feature_dir", type=str, default="clip_feat", help="feature dir path")
    args = ap.parse_args(argv)
    from mvlpt_amd import linear_probe as LP
    path = os.path.join(args.feature_dir, args.dataset)
    splits = [LP.load_split(path, s) for s in ("train", "val", "test")]
    LP.linear_probe(*splits, num_step=args.num_step, num_run=args.num_run, dataset=args.dataset, feature_dir=args.feature_dir,
                    report_dir="report", log=lambda *a: print(*a, flush=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
