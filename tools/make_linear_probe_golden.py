#!/usr/bin/env python
"""Regenerate tests/golden/linear_probe.npz: a recording of the reference's lpclip/linear_probe.py on a small synthetic feature set.

    python tools/make_linear_probe_golden.py --reference /path/to/reference_checkout

Also writes tests/golden/softmax_reg_optima.npz, the float64 minimisers the device fit tests compare against (no reference needed).

Needs the reference checkout and sklearn (the recording is of sklearn's fits); neither is needed by the tests.  The reference's script
is run unchanged (runpy) in a temporary directory with --num_step 3 --num_run 2, with sklearn.linear_model.LogisticRegression set to a
subclass that records every fit: C, the train / val rows (recovered by matching rows), the predictions on val and test, coef_,
intercept_, n_iter_.  The two report files are stored as text, the features as they were written.  Last, the same sweep is run with the
float64 Newton oracle as the fit, and the largest |accuracy - recorded accuracy| over the shots plus two test-set quanta is stored
as `sweep_margin` (percentage points): the margin tests/test_hip_linear_probe.py gives the device fits.
"""
import argparse
import contextlib
import io
import os
import runpy
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, D = 5, 16
ROWS = {"train": 20, "val": 6, "test": 40}      # rows per class
NUM_STEP, NUM_RUN = 3, 2
DATASET, FEATURE_DIR = "synthetic", "clip_feat"


def make_features(seed):
    rng = np.random.default_rng(seed)
    centres = 0.8 * rng.standard_normal((K, D))
    out = {}
    for split, per in ROWS.items():
        y = np.repeat(np.arange(K), per)
        rng.shuffle(y)
        x = (centres[y] + rng.standard_normal((len(y), D))).astype(np.float32)
        out[split] = (x.astype(np.float64), y.astype(np.int64))      # float64 as feat_extractor.py writes, fp32-representable
    return out


FIT_PROBLEMS = [(3, 4, 3), (20, 16, 5), (130, 68, 33)]      # (N, D, K) of the fit tests: one-shot, the fixture's size, ragged tiles
FIT_CS = [1e-7, 1e-4, 1e-2, 1.0, 1e2, 1e7]


def write_optima(path):
    """tests/golden/softmax_reg_optima.npz: the float64 Newton minimiser theta* and mu of every (problem, C) of the device fit tests
    (minutes of dense Hessians at the largest problem: solved once here, verified in tests/test_softmax_reg_ref.py by its gradient)."""
    import softmax_reg_ref as R
    out = {"problems": np.array(FIT_PROBLEMS), "Cs": np.array(FIT_CS)}
    for pi, (N, Dd, Kk) in enumerate(FIT_PROBLEMS):
        X, y = R.make_problem(N, Dd, Kk, seed=N)
        out[f"X{pi}"], out[f"y{pi}"] = X, y
        for ci, C in enumerate(FIT_CS):
            l2 = 1.0 / (C * N)
            theta = R.newton(X, y, Kk, l2)
            out[f"theta{pi}_{ci}"], out[f"mu{pi}_{ci}"] = theta, np.array(R.mu(theta, X, Kk, l2))
            print(f"optimum N {N} D {Dd} K {Kk} C {C:g}: F* {R.objective(theta, X, y, Kk, l2):.6f} mu {float(out[f'mu{pi}_{ci}']):.3e}")
    np.savez_compressed(path[:-4], **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of the reference project (lpclip/linear_probe.py is run from it); "
                    "without it only softmax_reg_optima.npz is written")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "linear_probe.npz"))
    args = ap.parse_args()
    write_optima(os.path.join(os.path.dirname(args.out), "softmax_reg_optima.npz"))
    if args.reference is None:
        return
    script = os.path.join(args.reference, "lpclip", "linear_probe.py")
    import sklearn
    import sklearn.linear_model
    from mvlpt_amd import linear_probe as LP
    import softmax_reg_ref as R

    feats = make_features(args.seed)
    row_of = {s: {feats[s][0][i].tobytes(): i for i in range(len(feats[s][0]))} for s in ("train", "val")}
    assert all(len(row_of[s]) == len(feats[s][0]) for s in row_of), "duplicate rows: indices cannot be recovered"
    test_x = feats["test"][0]
    rec = []
    Base = sklearn.linear_model.LogisticRegression

    class Recorder(Base):
        def fit(self, X, y, *a, **kw):
            super().fit(X, y, *a, **kw)
            self._rec = {"C": float(self.C), "train_idx": [row_of["train"][r.tobytes()] for r in X], "coef": self.coef_.copy(),
                         "intercept": self.intercept_.copy(), "n_iter": int(self.n_iter_[0]), "test_pred": Base.predict(self, test_x),
                         "val_idx": None, "val_pred": None}
            rec.append(self._rec)
            return self

        def predict(self, X):
            out = super().predict(X)
            if X.shape != test_x.shape:
                self._rec["val_idx"] = [row_of["val"][r.tobytes()] for r in X]
                self._rec["val_pred"] = out.copy()
            return out

    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        for split, (x, y) in feats.items():
            LP.save_split(os.path.join(tmp, FEATURE_DIR, DATASET), split, x, y)
        sklearn.linear_model.LogisticRegression = Recorder
        try:
            os.chdir(tmp)
            sys.argv = [script, "--dataset", DATASET, "--num_step", str(NUM_STEP), "--num_run", str(NUM_RUN), "--feature_dir", FEATURE_DIR]
            with contextlib.redirect_stdout(io.StringIO()):
                runpy.run_path(script, run_name="__main__")
            stem = os.path.join(tmp, "report", f"{FEATURE_DIR}_s{NUM_STEP}r{NUM_RUN}")
            details, summary = open(stem + "_details.txt").read(), open(stem + ".txt").read()
        finally:
            os.chdir(cwd)
            sys.argv = argv
            sklearn.linear_model.LogisticRegression = Base

        # the same sweep with the exact minimiser as the fit: how far two correct solvers' accuracies lie apart on this data
        class Exact:
            def __init__(self, X, y, C):
                self.classes, yi = np.unique(y, return_inverse=True)
                self.theta = R.newton(X, yi, len(self.classes), 1.0 / (C * len(y)))

            def predict(self, X):
                z, _, _ = R.probs(self.theta, X, len(self.classes))
                return self.classes[z.argmax(1)]

        res = LP.linear_probe(feats["train"], feats["val"], feats["test"], NUM_STEP, NUM_RUN, fit_fn=Exact, dataset=DATASET,
                              feature_dir=FEATURE_DIR, report_dir=os.path.join(tmp, "oracle_report"), log=lambda *a: None)
    assert all(r["val_idx"] is not None for r in rec)
    recorded = {int(l.split(",")[1].split()[0]): float(l.split("stat:")[1].split()[0]) for l in summary.splitlines()}
    gap = max(abs(res["summary"][s][0] - recorded[s]) for s in recorded)
    margin = gap + 2 * 100.0 / len(test_x)

    cat = lambda key: np.concatenate([np.asarray(r[key], np.int64) for r in rec])
    offs = lambda key: np.cumsum([0] + [len(r[key]) for r in rec]).astype(np.int64)
    np.savez_compressed(
        args.out[:-4] if args.out.endswith(".npz") else args.out,
        C=np.array([r["C"] for r in rec]), n_iter=np.array([r["n_iter"] for r in rec], np.int64),
        coef=np.stack([r["coef"] for r in rec]), intercept=np.stack([r["intercept"] for r in rec]),
        train_idx=cat("train_idx"), train_off=offs("train_idx"), val_idx=cat("val_idx"), val_off=offs("val_idx"),
        val_pred=cat("val_pred"), test_pred=np.stack([r["test_pred"] for r in rec]).astype(np.int64),
        details=np.array(details), summary=np.array(summary),
        train_x=feats["train"][0], train_y=feats["train"][1], val_x=feats["val"][0], val_y=feats["val"][1],
        test_x=feats["test"][0], test_y=feats["test"][1],
        num_step=np.array(NUM_STEP), num_run=np.array(NUM_RUN), dataset=np.array(DATASET), feature_dir=np.array(FEATURE_DIR),
        sweep_margin=np.array(margin), oracle_gap=np.array(gap), sklearn_version=np.array(sklearn.__version__), seed=np.array(args.seed))
    print(f"{len(rec)} fits recorded with sklearn {sklearn.__version__}; oracle gap {gap:.2f}, sweep margin {margin:.2f} points -> {args.out}")
    print(summary)


if __name__ == "__main__":
    main()
