"""Host side of the device evaluation (mvlpt_amd/evaluator.py), CPU only: the finishing functions fed with count vectors that numpy
computes, against scikit-learn's recorded figures (tests/golden/classification_eval.npz, tools/make_eval_golden.py) at |d| <= 1e-12
(a handful of double roundings on quantities in [0, 100]; sklearn averages with np.average), and the four ELEVATER finishers fed with
a numpy emulation of the rank kernel's integer formulation, `==` against mvlpt_amd/metrics.py."""
import numpy as np
import pytest

from mvlpt_amd import evaluator as E
from mvlpt_amd import metrics as M
from mvlpt_amd.config import get_cfg_default
from tests.golden_util import load_npz


def counts(y_true, y_pred, n):
    n_true, n_pred = np.bincount(y_true, minlength=n), np.bincount(y_pred, minlength=n)
    n_hit = np.bincount(y_true[y_true == y_pred], minlength=n)
    cmat = np.zeros((n, n), dtype=np.int64)
    np.add.at(cmat, (y_true, y_pred), 1)
    return n_true, n_pred, n_hit, cmat


def emulate(y_true, y_score, name):
    """the device route on the host: integer rank statistics per column, then the finishers"""
    y_score = np.asarray(y_score, dtype=np.float32)
    n, c = y_score.shape
    tar = M._target_matrix(y_true, c)
    if name == "accuracy":
        return E.finish_accuracy(np.bincount(y_true[np.argmax(y_score, axis=1) == y_true], minlength=c), n)
    if name == "mean-per-class":
        keep = np.any(tar != 0, axis=0)
        masked = np.where(keep[None, :], y_score, -np.inf)
        t, p = np.argmax(np.where(keep[None, :], tar, -1), axis=1), np.argmax(masked, axis=1)
        return E.finish_mean_per_class(np.bincount(t, minlength=c), np.bincount(t[t == p], minlength=c))
    stats = [E.rank_statistics_numpy(y_score[:, k], tar[:, k] == 1) for k in range(c)]
    n_pos, n_neg, twice_u = (np.array([s[i] for s in stats], dtype=np.int64) for i in range(3))
    if name == "roc_auc":
        return E.finish_roc_auc(n_pos, n_neg, twice_u)
    return E.finish_map(np.any(tar != 0, axis=0), np.stack([s[3] for s in stats]))


def test_config_keys_exist_with_dassl_defaults():
    cfg = get_cfg_default()
    assert cfg.TEST.PER_CLASS_RESULT is False and cfg.TEST.COMPUTE_CMAT is False
    assert cfg.TEST.DEVICE_METRICS is True
    cfg.merge_from_list(["TEST.PER_CLASS_RESULT", "True", "TEST.COMPUTE_CMAT", "True", "TEST.DEVICE_METRICS", "False"])
    assert cfg.TEST.PER_CLASS_RESULT is True and cfg.TEST.COMPUTE_CMAT is True and cfg.TEST.DEVICE_METRICS is False


def test_classification_figures_match_sklearn():
    g = load_npz("classification_eval")
    names = [str(n) for n in g["names"]]
    assert {"absent_truth", "pred_outside_truth"} <= set(names)
    for name in names:
        y_true, y_pred, n = g[f"{name}/y_true"], g[f"{name}/y_pred"], int(g[f"{name}/n_class"])
        n_true, n_pred, n_hit, cmat = counts(y_true, y_pred, n)
        res = E.classification_results(n_true, n_pred, n_hit, len(y_true))
        assert res["accuracy"] == 100.0 * int((y_true == y_pred).sum()) / len(y_true)
        assert res["error_rate"] == 100.0 - res["accuracy"]
        assert abs(res["macro_f1"] - 100.0 * float(g[f"{name}/macro_f1"])) <= 1e-12, name
        cm, labels = E.confusion_matrix(cmat, n_true, n_pred)
        assert np.array_equal(labels, np.union1d(y_true, y_pred))
        assert cm.shape == g[f"{name}/cmat"].shape and np.abs(cm - g[f"{name}/cmat"]).max() <= 1e-12, name
        rows, mean_acc = E.perclass_table(n_true, n_hit, {k: f"c{k}" for k in range(n)})
        assert [r[0] for r in rows] == np.unique(y_true).tolist()
        want = [100.0 * int(((y_true == k) & (y_pred == k)).sum()) / int((y_true == k).sum()) for k in np.unique(y_true)]
        assert [r[4] for r in rows] == want and mean_acc == float(np.mean(want))


def test_a_label_set_with_classes_absent_from_truth_changes_the_macro_average():
    """the two sets the fixture must hold: averaging over all classes instead of np.unique(y_true) would fail here"""
    g = load_npz("classification_eval")
    for name in ("absent_truth", "pred_outside_truth"):
        y_true, y_pred, n = g[f"{name}/y_true"], g[f"{name}/y_pred"], int(g[f"{name}/n_class"])
        assert len(np.unique(y_true)) < n
    y_true, y_pred = g["pred_outside_truth/y_true"], g["pred_outside_truth/y_pred"]
    assert len(np.setdiff1d(y_pred, y_true)) > 0
    assert g["pred_outside_truth/cmat"].shape[0] == len(np.union1d(y_true, y_pred)) > len(np.unique(y_true))


def test_elevater_finishers_equal_metrics_py_on_the_golden_cases():
    g = load_npz("metrics")
    assert len(g["cases"]) == 6
    for i in g["cases"]:
        s, y, oh = g[f"c{i}_score"], g[f"c{i}_y"], g[f"c{i}_onehot"]
        assert emulate(y, s, "accuracy") == M.accuracy(y, s)
        assert emulate(oh, s, "mean-per-class") == M.balanced_accuracy_score(oh, s)
        assert emulate(y, s, "mean-per-class") == M.balanced_accuracy_score(y, s)
        assert emulate(oh, s, "11point_mAP") == M.map_11_points(oh, s)
        if f"c{i}_roc_auc" in g:
            assert emulate(oh, s, "roc_auc") == M.roc_auc(oh, s)
        else:
            with pytest.raises(ValueError, match="Only one class present"):
                emulate(oh, s, "roc_auc")


@pytest.mark.parametrize("kind", ["continuous", "quantised", "equal", "zeros"])
def test_integer_formulation_equals_metrics_py_on_ties(kind):
    rng = np.random.default_rng({"continuous": 0, "quantised": 1, "equal": 2, "zeros": 3}[kind])
    for n, c in ((1, 1), (2, 2), (3, 7), (65, 3), (257, 20)):
        s = rng.standard_normal((n, c)).astype(np.float32)
        if kind == "quantised":
            s = np.round(s * 1.5).astype(np.float32) / 2
        elif kind == "equal":
            s[:] = 0.25
        elif kind == "zeros":
            s = rng.choice(np.array([0.0, -0.0, 1.0], dtype=np.float32), (n, c))
        y = rng.integers(0, c, n)
        oh = np.eye(c, dtype=np.float32)[y]
        assert emulate(oh, s, "11point_mAP") == M.map_11_points(oh, s)
        assert emulate(oh, s, "mean-per-class") == M.balanced_accuracy_score(oh, s)
        try:
            want = M.roc_auc(oh, s)
        except ValueError:
            with pytest.raises(ValueError):
                emulate(oh, s, "roc_auc")
        else:
            assert emulate(oh, s, "roc_auc") == want
