"""The float64 oracle of the linear probe (tests/softmax_reg_ref.py) against itself and against recorded sklearn fits (CPU).

tests/golden/linear_probe.npz holds the 130 fits sklearn 1.7.2 made when the reference's lpclip/linear_probe.py ran on a synthetic
feature set (tools/make_linear_probe_golden.py).  Under the oracle's F with l2 = 1 / (C N) every recorded solution must meet sklearn's
own stopping rule max|grad F| <= 1e-4 and lie above the oracle's minimum: that pins the objective to the real thing.
"""
import os

import numpy as np
import pytest

from tests import softmax_reg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(GOLDEN, "linear_probe.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def optima():
    with np.load(os.path.join(GOLDEN, "softmax_reg_optima.npz")) as f:
        return {k: f[k] for k in f.files}


def test_gradient_and_hessian_against_differences():
    X, y = R.make_problem(12, 8, 4, seed=5)
    K, l2 = 4, 0.03
    theta = np.random.default_rng(1).standard_normal(K * 8 + K) * 0.3
    g, H = R.gradient(theta, X, y, K, l2), R.hessian(theta, X, K, l2)
    h = 1e-5
    for j in range(0, len(theta), 5):
        e = np.zeros_like(theta)
        e[j] = h
        fd = (R.objective(theta + e, X, y, K, l2) - R.objective(theta - e, X, y, K, l2)) / (2 * h)
        assert abs(fd - g[j]) < 1e-9
        hd = (R.gradient(theta + e, X, y, K, l2) - R.gradient(theta - e, X, y, K, l2)) / (2 * h)
        assert np.abs(hd - H[:, j]).max() < 1e-9
    assert np.abs(H - H.T).max() < 1e-15
    v = R.null_direction(K, 8)
    assert np.abs(H @ v).max() < 1e-15                                   # F does not change under b + c 1
    assert abs(R.objective(theta + 3.0 * np.sqrt(K) * v, X, y, K, l2) - R.objective(theta, X, y, K, l2)) < 1e-14


def test_zero_theta_is_log_k():
    X, y = R.make_problem(9, 4, 3, seed=2)
    assert abs(R.objective(np.zeros(15), X, y, 3, 0.5) - np.log(3)) < 1e-15
    _, p, _ = R.probs(np.zeros(15), X, 3)
    assert np.array_equal(p, np.full((9, 3), 1 / 3))


def test_recorded_sklearn_solutions_meet_the_stopping_rule_and_lie_above_the_minimum(fx):
    K = fx["coef"].shape[1]
    worst, solved = 0.0, {}
    for n in range(len(fx["C"])):
        rows = fx["train_idx"][fx["train_off"][n]:fx["train_off"][n + 1]]
        X, y = fx["train_x"][rows], fx["train_y"][rows]
        l2 = 1.0 / (fx["C"][n] * len(rows))
        theta = np.concatenate([fx["coef"][n].ravel(), fx["intercept"][n]])
        gmax = np.abs(R.gradient(theta, X, y, K, l2)).max()
        worst = max(worst, gmax)
        assert gmax <= 1e-4, (n, fx["C"][n], gmax)
        key = (rows.tobytes(), float(fx["C"][n]))
        if key not in solved:
            solved[key] = R.objective(R.newton(X, y, K, l2), X, y, K, l2)
        assert R.objective(theta, X, y, K, l2) >= solved[key]
    print(f"{len(fx['C'])} recorded fits: worst max|grad F| {worst:.2e} (sklearn's tol 1e-4)")


def test_stored_optima_are_stationary_and_small_ones_reproduce(optima):
    for pi, (N, D, K) in enumerate(optima["problems"]):
        X, y = R.make_problem(int(N), int(D), int(K), seed=int(N))
        assert np.array_equal(X, optima[f"X{pi}"]) and np.array_equal(y, optima[f"y{pi}"])
        for ci, C in enumerate(optima["Cs"]):
            l2 = 1.0 / (C * N)
            theta = optima[f"theta{pi}_{ci}"]
            assert np.abs(R.gradient(theta, X, y, int(K), l2)).max() < 1e-13
            assert abs(theta[K * D:].mean()) < 1e-12
            if N <= 20:
                again = R.newton(X, y, int(K), l2)
                mu = float(optima[f"mu{pi}_{ci}"])
                assert np.linalg.norm(again - theta) <= 2 * 2e-13 * np.sqrt(len(theta)) / mu + 1e-12
                assert abs(R.mu(theta, X, int(K), l2) - mu) <= 1e-6 * mu + 1e-18


def test_fp32_restatement_sits_inside_the_evaluation_bounds():
    X, y = R.make_problem(37, 24, 5, seed=3)
    theta = (np.random.default_rng(0).standard_normal(5 * 24 + 5) * 0.5).astype(np.float32)
    l2 = 1e-3
    g, st = R.eval_fp32(theta, X, y, 5, l2)
    b = R.eval_bounds(theta, X, y, 5, l2)
    assert abs(st[0] - R.objective(theta, X, y, 5, l2)) <= b["F"]
    assert np.all(np.abs(g - R.gradient(theta, X, y, 5, l2)) <= b["grad"])
