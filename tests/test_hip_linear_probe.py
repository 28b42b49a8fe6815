"""The linear probe end to end on the device (-m gpu): predictions where the oracle decides them, the sweep over C on the recorded
feature set with device fits, and feature extraction through the tiny tower.

No test asks for prediction or accuracy EQUALITY with sklearn: at weak regularisation two correct solvers differ on a few per cent of
the predictions (DESIGN.md row j).  The sweep's accuracies get the margin measured on the CPU with the float64 oracle as the fit
(`sweep_margin` of tests/golden/linear_probe.npz, tools/make_linear_probe_golden.py).
"""
import os

import numpy as np
import pytest
import torch

from tests import softmax_reg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "linear_probe.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("Cw", [0.01, 1.0])
def test_predictions_where_they_are_decidable(fx, Cw):
    """predict equals the oracle's arg-max on every test row whose oracle margin exceeds twice what the fit's displacement and the
    fp32 logits can move a logit: |x|_1 |dW|_max + |db|_max with |theta - theta*|_2 <= 2 |grad F(theta)|_2 / mu for both, plus the
    logit bound of the evaluation.  At most 5 % of the rows may be left out (the oracle alone decides that)."""
    from mvlpt_amd.linear_probe import SoftmaxRegression
    X, y, Xt = fx["train_x"], fx["train_y"], fx["test_x"]
    N, D = X.shape
    K, l2 = 5, 1.0 / (Cw * N)
    ts = R.newton(X, y, K, l2)
    mu = R.mu(ts, X, K, l2)
    clf = SoftmaxRegression(C=Cw, tol=1e-6, device=DEV).fit(X, y)
    assert clf.status_ == "gtol"
    th = np.concatenate([clf.coef_.ravel(), clf.intercept_]).astype(np.float64)
    disp = 2 * np.linalg.norm(R.gradient(th, X, y, K, l2)) / mu
    assert np.linalg.norm(th - ts) <= disp
    z, _, _ = R.probs(ts, Xt, K)
    top2 = np.sort(z, 1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    move = np.abs(Xt).sum(1) * disp + disp + R.logit_bound(th, Xt, K).max(1)
    decided = margin > 2 * move
    print(f"C {Cw:g}: displacement bound {disp:.2e}, smallest margin {margin.min():.2e}, {decided.sum()} / {len(Xt)} rows decided")
    assert decided.mean() >= 0.95
    pred, dm = clf.predict(Xt, return_margin=True)
    assert np.array_equal(pred[decided], z.argmax(1)[decided])
    assert np.all(np.abs(dm - margin) <= 2 * move + R.U * margin)


def test_sweep_on_the_recorded_features_with_device_fits(fx, tmp_path):
    from mvlpt_amd import linear_probe as LP
    fits = []

    def fit(X, y, Cw):
        clf = LP.SoftmaxRegression(C=Cw, max_iter=1000, device=DEV).fit(X, y)
        fits.append((Cw, clf.status_, clf.n_iter_))
        return clf

    num_step, num_run = int(fx["num_step"]), int(fx["num_run"])
    res = LP.linear_probe((fx["train_x"], fx["train_y"]), (fx["val_x"], fx["val_y"]), (fx["test_x"], fx["test_y"]), num_step, num_run,
                          fit_fn=fit, dataset="synthetic", feature_dir="clip_feat", report_dir=str(tmp_path), log=lambda *a: None)
    assert len(fits) == res["fits"] == 5 * num_run * (7 + 2 * num_step)
    bad = [f for f in fits if f[1] != "gtol"]
    assert not bad, bad[:5]
    details = open(tmp_path / f"clip_feat_s{num_step}r{num_run}_details.txt").read().splitlines()
    summary = open(tmp_path / f"clip_feat_s{num_step}r{num_run}.txt").read().splitlines()
    assert len(details) == 5 * num_run * num_step and len(summary) == 5
    for line in details:
        name, seed, shot, weight, acc = [t.strip() for t in line.split(",")]
        assert name == "synthetic" and seed.startswith("seed ") and shot.endswith(" shot")
        assert float(weight.split()[1]) > 0 and 0 <= float(acc.split()[1]) <= 100
    recorded = {int(l.split(",")[1].split()[0]): float(l.split("stat:")[1].split()[0]) for l in str(fx["summary"]).splitlines()}
    margin = float(fx["sweep_margin"])
    for line in summary:
        shot, mean = int(line.split(",")[1].split()[0]), float(line.split("stat:")[1].split()[0])
        print(f"{shot} shot: {mean:.2f} (recorded {recorded[shot]:.2f}, margin {margin:.2f}); most iterations {max(f[2] for f in fits)}")
        assert abs(mean - recorded[shot]) <= margin + 0.005        # both figures are printed with two decimals


def test_extract_features_rows_are_encode_image_rows():
    from mvlpt_amd import linear_probe as LP
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    arch = ARCHS["tiny"]
    clip = FrozenCLIP(make_state_dict(arch, seed=3), compute_dtype="fp16", device=DEV)
    g = torch.Generator().manual_seed(0)
    sizes = [3, 1, 5, 2]
    batches = [(torch.randn(b, 3, arch.image_resolution, arch.image_resolution, generator=g), torch.arange(b) + 10 * k)
               for k, b in enumerate(sizes)]
    feats, labels = LP.extract_features(clip, iter(batches))
    assert feats.shape == (sum(sizes), arch.embed_dim) and feats.dtype == np.float32 and labels.dtype == np.int64
    assert labels.tolist() == [int(v) for _, l in batches for v in l]
    want = np.concatenate([clip.encode_image(im).cpu().numpy() for im, _ in batches])
    assert feats.tobytes() == want.tobytes()
    assert np.abs(np.linalg.norm(feats, axis=1) - 1).max() > 1e-3          # un-normalised, as clip_model.visual returns them
