"""Host side of the linear probe (CPU): few-shot sampling, the search over C, the report and feature files, argument errors, and the
L-BFGS driver on a numpy restatement of the device evaluation.  The search is replayed against the recording of the reference's
lpclip/linear_probe.py in tests/golden/linear_probe.npz: every fit must be asked with the recorded C (==) and rows, in order.
"""
import os

import numpy as np
import pytest
import torch

from mvlpt_amd import linear_probe as LP
from tests import softmax_reg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "linear_probe.npz")) as f:
        return {k: f[k] for k in f.files}


def fit_schedule(fx):
    """(shot, seed) of every recorded fit: 7 + 2 * num_step fits per pair, shots outermost."""
    per = 7 + 2 * int(fx["num_step"])
    pairs = [(shot, seed) for shot in (1, 2, 4, 8, 16) for seed in range(1, int(fx["num_run"]) + 1)]
    assert len(fx["C"]) == per * len(pairs)
    return per, pairs


def test_sampling_is_bit_exact(fx):
    per, pairs = fit_schedule(fx)
    for p, (shot, seed) in enumerate(pairs):
        state = np.random.RandomState(seed)
        classes = np.unique(fx["train_y"])
        tr = LP.sample_few_shot(fx["train_y"], shot, state, classes)
        va = LP.sample_few_shot(fx["val_y"], LP.VAL_SHOTS[shot], state, classes)
        for n in range(p * per, (p + 1) * per):
            assert np.array_equal(tr, fx["train_idx"][fx["train_off"][n]:fx["train_off"][n + 1]])
            assert np.array_equal(va, fx["val_idx"][fx["val_off"][n]:fx["val_off"][n + 1]])


def test_search_replays_the_reference_call_for_call(fx, tmp_path):
    calls = []

    class Replay:
        def __init__(self, n):
            self.n = n

        def predict(self, X):
            if X.shape == fx["test_x"].shape and np.array_equal(X, fx["test_x"]):
                return fx["test_pred"][self.n]
            rows = fx["val_idx"][fx["val_off"][self.n]:fx["val_off"][self.n + 1]]
            assert np.array_equal(X, fx["val_x"][rows])
            return fx["val_pred"][fx["val_off"][self.n]:fx["val_off"][self.n + 1]]

    def replay(X, y, C):
        n = len(calls)
        rows = fx["train_idx"][fx["train_off"][n]:fx["train_off"][n + 1]]
        assert C == fx["C"][n], (n, C, fx["C"][n])
        assert np.array_equal(X, fx["train_x"][rows]) and np.array_equal(y, fx["train_y"][rows])
        calls.append(C)
        return Replay(n)

    num_step, num_run = int(fx["num_step"]), int(fx["num_run"])
    res = LP.linear_probe((fx["train_x"], fx["train_y"]), (fx["val_x"], fx["val_y"]), (fx["test_x"], fx["test_y"]), num_step, num_run,
                          fit_fn=replay, dataset=str(fx["dataset"]), feature_dir=str(fx["feature_dir"]),
                          report_dir=str(tmp_path / "report"), log=lambda *a: None)
    assert len(calls) == len(fx["C"]) == res["fits"]
    stem = tmp_path / "report" / f"{fx['feature_dir']}_s{num_step}r{num_run}"
    assert open(str(stem) + "_details.txt").read() == str(fx["details"])
    assert open(str(stem) + ".txt").read() == str(fx["summary"])
    # the (c_left, c_right, c_final) of every round are the recorded fits' C: left, right in call order, the winner in the report
    per, pairs = fit_schedule(fx)
    for r, (shot, seed, step, c_left, c_right, c_final, _) in enumerate(res["trace"]):
        base = (r // num_step) * per + 7 + 2 * step
        assert (c_left, c_right) == (fx["C"][base], fx["C"][base + 1]) and c_final in (c_left, c_right)
    weights = [float(l.split("weight ")[1].split(",")[0]) for l in str(fx["details"]).splitlines()]
    assert weights == [float(t[5]) for t in res["trace"]]


def test_left_branch_wins_a_tie_and_first_peak_is_taken(tmp_path):
    asked = []

    class Const:
        def predict(self, X):
            return np.zeros(len(X), np.int64)

    def fit(X, y, C):
        asked.append(C)
        return Const()

    y = np.repeat(np.arange(3), 4)
    X = np.zeros((12, 4))
    LP.linear_probe((X, y), (X, y), (X, y), num_step=2, num_run=1, shots=(1,), fit_fn=fit, report_dir=str(tmp_path), log=lambda *a: None)
    assert asked[:7] == LP.SEARCH_LIST
    assert asked[7:9] == [1e-1 * 1e6, 1e1 * 1e6]                       # all accuracies equal: argmax takes the first, 1e6
    lo, hi = np.log10(asked[7]), 0.5 * (np.log10(asked[8]) + np.log10(asked[7]))
    assert asked[9:11] == [np.power(10, lo), np.power(10, hi)]         # the left end won the tie: the interval moves left


def test_npz_round_trip_with_the_reference_keys(tmp_path):
    f = np.arange(24, dtype=np.float32).reshape(6, 4)
    l = np.array([0, 1, 2, 0, 1, 2])
    path = LP.save_split(str(tmp_path / "feat" / "Data"), "train", f.tolist(), l.tolist())      # lists, as feat_extractor.py passes
    assert path.endswith("train.npz") and os.path.isfile(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["feature_list", "label_list"]
    f2, l2 = LP.load_split(str(tmp_path / "feat" / "Data"), "train")
    assert np.array_equal(f2, f) and np.array_equal(l2, l)


def test_value_errors():
    X = np.zeros((6, 8), np.float32)
    with pytest.raises(ValueError, match="3 classes"):
        LP.SoftmaxRegression().fit(X, np.array([0, 1, 0, 1, 0, 1]))
    with pytest.raises(ValueError, match="multiple of 4"):
        LP.SoftmaxRegression().fit(np.zeros((6, 6), np.float32), np.array([0, 1, 2, 0, 1, 2]))
    with pytest.raises(ValueError, match="fewer than"):
        LP.sample_few_shot(np.array([0, 0, 1, 2, 2]), 2, np.random.RandomState(1))
    with pytest.raises(ValueError):
        LP.SoftmaxRegression().fit(X, np.array([0, 1, 2]))


@pytest.mark.parametrize("C", [1e-7, 1e-4, 1e-2, 1.0, 1e2, 1e7])
@pytest.mark.parametrize("tol", [1e-4, 1e-6])
def test_driver_converges_on_the_fp32_restatement(C, tol):
    """The L-BFGS driver with the device's precision classes restated in numpy (fp32 logits, double row stage): it must stop by the
    gradient rule at every C, the strong regularisation included where an fp32 loss stalls a line search."""
    with np.load(os.path.join(GOLDEN, "softmax_reg_optima.npz")) as f:
        X, y, Cs = f["X1"], f["y1"], list(f["Cs"])
        ts, mu = f[f"theta1_{Cs.index(C)}"], float(f[f"mu1_{Cs.index(C)}"])
    N, D = X.shape
    K, l2 = 5, 1.0 / (C * N)

    def ev(theta, d):
        g, st = R.eval_fp32(theta.numpy(), X, y, K, l2, None if d is None else d.numpy())
        return torch.from_numpy(g), st

    theta, n_iter, status, st = LP.lbfgs_minimize(ev, torch.zeros(K * D + K), tol, 1000)
    assert status == "gtol" and n_iter < 100 and st[1] <= tol
    th = R.centre(theta.numpy(), K, D)
    g = R.gradient(th, X, y, K, l2)
    assert np.abs(g).max() <= tol + R.eval_bounds(th, X, y, K, l2)["grad"].max()
    gap = R.objective(th, X, y, K, l2) - R.objective(ts, X, y, K, l2)
    assert -1e-15 <= gap <= g @ g / mu + 1e-15
    if C <= 1:
        assert np.linalg.norm(th - ts) <= 2 * np.linalg.norm(g) / mu


def test_driver_passes_the_rounding_floor_of_a_coarse_objective():
    """An objective that resolves only 1e-7 (rounded to fp32 here), heavily penalised coordinates next to a flat one: close to the
    minimiser no step lowers F visibly and the flat coordinate needs steps far longer than the scaled direction.  The slope test must
    carry the search to the gradient rule, and a step that does not move fp32 theta must never be taken for progress."""
    h = np.array([500.0, 500.0, 500.0, 500.0, 0.2])
    target = np.array([1e-3, -2e-3, 5e-4, 0.0, 1.0])
    events = []

    def ev(theta, d):
        e = theta.double().numpy() - target
        g = (h * e).astype(np.float32)
        F = float(np.float32(1.6 + 0.5 * float(e @ (h * e))))
        g64 = g.astype(np.float64)
        return torch.from_numpy(g), [F, float(np.abs(g64).max()), 0.0 if d is None else float(g64 @ d.double().numpy()), float(g64 @ g64)]

    theta, n_iter, status, st = LP.lbfgs_minimize(ev, torch.zeros(5), 1e-6, 200, callback=lambda *a: events.append(a[1]))
    assert status == "gtol" and st[1] <= 1e-6 and n_iter < 60
    assert "wolfe" in events                              # the rounding floor was reached and passed
    assert np.abs(theta.numpy() - target).max() < 1e-5
