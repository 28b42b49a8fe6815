"""Writes tests/golden/classification_eval.npz: seeded (y_true, y_pred) label sets with the figures scikit-learn records for them,

    f1_score(y_true, y_pred, average="macro", labels=np.unique(y_true))          (Dassl's macro_f1 before the factor 100)
    confusion_matrix(y_true, y_pred, normalize="true")                            (Dassl's TEST.COMPUTE_CMAT)

so that the host finishing functions of mvlpt_amd/evaluator.py are pinned to sklearn without sklearn being needed to run the tests.
Needs scikit-learn (recorded with 1.7.2; the version that wrote the file is stored in it).  Usage: python tools/make_eval_golden.py"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "classification_eval.npz")

# name -> (samples, classes, how the labels are drawn)
SETS = {
    "dense": (400, 7, "every class occurs in truth and in prediction"),
    "absent_truth": (300, 12, "classes 3, 7 and 11 never occur in truth and are never predicted"),
    "pred_outside_truth": (300, 10, "classes 2 and 9 never occur in truth but are predicted"),
    "single_class": (50, 4, "one true class only"),
    "tiny": (3, 5, "three samples"),
}


def draw(name, rng):
    n, c, _ = SETS[name]
    if name == "dense":
        y_true = rng.integers(0, c, n)
        y_pred = np.where(rng.random(n) < 0.6, y_true, rng.integers(0, c, n))
    elif name == "absent_truth":
        present = np.array([k for k in range(c) if k not in (3, 7, 11)])
        y_true = rng.choice(present, n)
        y_pred = np.where(rng.random(n) < 0.5, y_true, rng.choice(present, n))
    elif name == "pred_outside_truth":
        present = np.array([k for k in range(c) if k not in (2, 9)])
        y_true = rng.choice(present, n)
        y_pred = np.where(rng.random(n) < 0.5, y_true, rng.integers(0, c, n))
        y_pred[:4] = [2, 9, 2, 9]
    elif name == "single_class":
        y_true = np.full(n, 2)
        y_pred = rng.integers(0, c, n)
    else:
        y_true, y_pred = np.array([4, 0, 4]), np.array([4, 1, 0])
    return y_true.astype(np.int64), y_pred.astype(np.int64)


def main():
    import sklearn
    from sklearn.metrics import confusion_matrix, f1_score
    out = {"sklearn_version": np.array(sklearn.__version__), "names": np.array(sorted(SETS))}
    for i, name in enumerate(sorted(SETS)):
        y_true, y_pred = draw(name, np.random.default_rng(1000 + i))
        out[f"{name}/n_class"] = np.array(SETS[name][1])
        out[f"{name}/y_true"], out[f"{name}/y_pred"] = y_true, y_pred
        out[f"{name}/macro_f1"] = np.array(f1_score(y_true, y_pred, average="macro", labels=np.unique(y_true)), dtype=np.float64)
        out[f"{name}/cmat"] = confusion_matrix(y_true, y_pred, normalize="true").astype(np.float64)
    np.savez(OUT, **out)
    print(f"wrote {OUT} with scikit-learn {sklearn.__version__}")


if __name__ == "__main__":
    main()
