"""Softmax-regression kernels on the device (-m gpu): mvlpt_op_softmax_reg_eval / _predict and SoftmaxRegression.fit against the float64
oracle of tests/softmax_reg_ref.py.

Every bound is derived from float64 magnitudes in the oracle module (u = 2^-24; the logits are a D-term fp32 chain, the row stage is
double, R is rounded once, the gradient is an N-term fp32 chain whose slices are added in double); nothing is tuned to what the device
returns.  Each test prints its worst error over its bound.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import softmax_reg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, D, K).  The kernels tile 128 x 128 outputs with reduction chunks of 16, pad the class pitch of Z to a multiple of 4, and split the
# rows of the gradient product into ceil(N / rows) slices, rows = max(32, roundup16(ceil(N / max(1, 256 / output tiles)))).
SHAPES = [
    (1, 4, 2), (3, 4, 3), (37, 24, 5), (130, 68, 33), (515, 512, 101),      # the issue's list: smallest, odd, ragged in all three
    (128, 8, 3), (129, 8, 3),          # one and two row tiles of the logits product
    (40, 8, 128), (40, 8, 129),        # one and two class tiles (both products), class pitch 128 / 132, 256 / 128 wanted slices
    (40, 128, 3), (40, 132, 3),        # one and two feature tiles of the gradient product
    (32, 4, 3), (33, 4, 3),            # one and two row slices (the second slice holds a single row)
    (8192, 4, 3), (8193, 4, 3),        # 256 slices of 32 rows, the cap; one row more: 171 slices of 48 rows
]
THETAS = ["zero", "unit", "spread"]
SENT = -12345.0


def problem(N, D, K, kind, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    y = rng.integers(0, K, N)
    if kind == "zero":
        theta = np.zeros(K * D + K, np.float32)
    else:
        W = rng.standard_normal((K, D)) / np.sqrt(D)
        theta = np.concatenate([W.ravel(), rng.standard_normal(K)]).astype(np.float32)
        if kind == "spread":            # row 0 gets a logit 80 above the rest: without the max subtraction exp overflows fp32
            w0 = theta[:D].astype(np.float64)
            X[0] = (80.0 * w0 / (w0 @ w0)).astype(np.float32)
    d = rng.standard_normal(K * D + K).astype(np.float32)
    return X, y, theta, d


def device_eval(X, y, theta, l2, d):
    from mvlpt_amd import engine as E
    N, D = X.shape
    K = theta.size // (D + 1)
    n = theta.size
    gfull = torch.full((n + 8,), SENT, device=DEV)
    sfull = torch.full((4 + 2,), SENT, device=DEV, dtype=torch.float64)
    ws = E.softmax_reg_workspace(N, D, K, DEV)
    Xd, yd, td = torch.tensor(X).to(DEV), torch.tensor(y.astype(np.int32)).to(DEV), torch.tensor(theta).to(DEV)
    dd = None if d is None else torch.tensor(d).to(DEV)
    E.op_softmax_reg_eval(Xd, yd, td, l2, dir=dd, grad=gfull[:n], stats=sfull[:4], ws=ws)
    torch.cuda.synchronize()
    assert bool((gfull[n:] == SENT).all()) and bool((sfull[4:] == SENT).all()), "guard elements behind grad / stats were written"
    ldz = (K + 3) // 4 * 4
    Rdev = ws.view(torch.float32)[:N * ldz].reshape(N, ldz)[:, :K].cpu().numpy()
    return gfull[:n].cpu().numpy(), sfull[:4].cpu().numpy(), Rdev


@pytest.mark.parametrize("kind", THETAS)
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_eval_against_float64(shape, kind):
    N, D, K = shape
    X, y, theta, d = problem(N, D, K, kind, seed=N * 7 + D + K)
    l2 = 1.0 / (0.5 * N)
    g, st, Rdev = device_eval(X, y, theta, l2, d)
    b = R.eval_bounds(theta, X, y, K, l2)
    g64, F64 = R.gradient(theta, X, y, K, l2), R.objective(theta, X, y, K, l2)
    _, p, _ = R.probs(theta, X, K)
    R64 = p.copy()
    R64[np.arange(N), y] -= 1.0
    R64 /= N
    eg, eR, eF = np.abs(g - g64), np.abs(Rdev - R64), abs(st[0] - F64)
    tiny = 1e-300
    print(f"{shape} {kind}: F {eF / b['F']:.3f}  R {(eR / (b['R'] + tiny)).max():.3f}  grad {(eg / (b['grad'] + tiny)).max():.3f} of the bound")
    assert eF <= b["F"]
    assert np.all(eR <= b["R"])
    assert np.all(eg <= b["grad"])
    if kind == "zero":
        assert abs(st[0] - np.log(K)) <= b["F"] and np.all(np.abs(Rdev - R64) <= R.U / N)      # p = 1 / K, F = log K
    # the statistics are those of the gradient the call returned (double sums: 1e-13 of the absolute terms) ...
    gd_, d_ = g.astype(np.float64), d.astype(np.float64)
    assert st[1] == np.abs(gd_).max()
    assert abs(st[2] - gd_ @ d_) <= 1e-13 * (np.abs(gd_) @ np.abs(d_)) + 1e-300
    assert abs(st[3] - gd_ @ gd_) <= 1e-13 * (gd_ @ gd_) + 1e-300
    # ... and therefore inside the gradient's bound of the oracle's
    assert abs(st[1] - np.abs(g64).max()) <= b["grad"].max()
    assert abs(st[2] - g64 @ d_) <= b["grad"] @ np.abs(d_) + 1e-13 * (np.abs(g64) @ np.abs(d_))
    assert abs(st[3] - g64 @ g64) <= (2 * np.abs(g64) + b["grad"]) @ b["grad"] + 1e-13 * (g64 @ g64)


def test_eval_without_direction_reports_zero():
    X, y, theta, _ = problem(37, 24, 5, "unit", seed=1)
    _, st, _ = device_eval(X, y, theta, 0.01, None)
    assert st[2] == 0.0


def test_two_calls_are_bit_equal_also_after_work_on_another_stream():
    X, y, theta, d = problem(515, 512, 101, "unit", seed=11)
    g1, s1, _ = device_eval(X, y, theta, 1e-3, d)
    g2, s2, _ = device_eval(X, y, theta, 1e-3, d)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        a = torch.randn(512, 512, device=DEV)
        for _ in range(4):
            a = torch.tanh(a @ a)
    g3, s3, _ = device_eval(X, y, theta, 1e-3, d)
    torch.cuda.synchronize()
    for g, s in ((g2, s2), (g3, s3)):
        assert g1.tobytes() == g.tobytes() and s1.tobytes() == s.tobytes()


PREDICT_SHAPES = [(37, 24, 5), (130, 68, 33), (515, 512, 101), (129, 8, 129)]


@pytest.mark.parametrize("shape", PREDICT_SHAPES, ids=[str(s) for s in PREDICT_SHAPES])
def test_predict_where_the_oracle_decides_ties_and_margin(shape):
    from mvlpt_amd import _lib
    from mvlpt_amd import engine as E
    N, D, K = shape
    X, _, theta, _ = problem(N, D, K, "unit", seed=5 * N + K)
    z0, _, _ = R.probs(theta, X, K)
    i, j = int(np.bincount(z0[:, :K - 1].argmax(1)).argmax()), K - 1      # the last class becomes a bitwise copy of the most frequent
                                                                          # winner among the others: exact ties, on many rows
    theta[j * D:(j + 1) * D] = theta[i * D:(i + 1) * D]
    theta[K * D + j] = theta[K * D + i]
    z, _, _ = R.probs(theta, X, K)
    dz = R.logit_bound(theta, X, K).max(1)
    top2 = np.sort(z, 1)[:, -2:]
    margin64 = top2[:, 1] - top2[:, 0]
    Xd, td = torch.tensor(X).to(DEV), torch.tensor(theta).to(DEV)
    pfull = torch.full((N + 4,), -77, device=DEV, dtype=torch.int32)
    mfull = torch.full((N + 4,), SENT, device=DEV)
    ws = E.softmax_reg_workspace(N, D, K, DEV)
    _lib.check(_lib.lib.mvlpt_op_softmax_reg_predict(C.c_void_p(Xd.data_ptr()), C.c_void_p(td.data_ptr()), N, D, K,
                                                      C.c_void_p(pfull.data_ptr()), C.c_void_p(mfull.data_ptr()),
                                                      C.c_void_p(ws.data_ptr()), ws.numel() * 8,
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), None, "predict")
    torch.cuda.synchronize()
    assert bool((pfull[N:] == -77).all()) and bool((mfull[N:] == SENT).all()), "guard elements behind pred / margin were written"
    pred, margin = pfull[:N].cpu().numpy(), mfull[:N].cpu().numpy()
    assert pred.min() >= 0 and pred.max() < K and not np.any(pred == j)         # the copy never wins: ties go to the lowest index
    zd = z.copy()
    zd[:, j] = -np.inf                                    # the order among the DISTINCT classes
    t2 = np.sort(zd, 1)[:, -2:]
    decided = (t2[:, 1] - t2[:, 0]) > 2 * dz
    assert decided.sum() >= N // 2
    assert np.array_equal(pred[decided], zd.argmax(1)[decided])
    tied = decided & (zd.argmax(1) == i)
    assert tied.any() and np.all(margin[tied] == 0.0)     # the winner and its copy have the same bits
    err = np.abs(margin - margin64)
    bound = 2 * dz + R.U * np.abs(margin64)
    print(f"{shape}: {decided.sum()} / {N} rows decided, {tied.sum()} tied, margin {(err / bound).max():.3f} of the bound")
    assert np.all(err <= bound)
    assert np.array_equal(E.op_softmax_reg_predict(Xd, td).cpu().numpy(), pred)


def test_argument_errors_leave_a_message():
    from mvlpt_amd import _lib
    out = C.c_size_t()
    for N, D, K in [(0, 4, 3), (5, 4, 1), (5, 6, 3), (5, 0, 3)]:
        assert _lib.lib.mvlpt_softmax_reg_workspace_bytes(N, D, K, C.byref(out)) == _lib.ERR_ARG
        assert "softmax_reg_workspace_bytes" in _lib.last_error(None)
    X, y, theta, _ = problem(5, 8, 3, "unit", seed=0)
    from mvlpt_amd import engine as E
    with pytest.raises(RuntimeError, match="workspace"):
        E.op_softmax_reg_eval(torch.tensor(X).to(DEV), torch.tensor(y.astype(np.int32)).to(DEV), torch.tensor(theta).to(DEV), 0.1,
                              ws=torch.empty(2, device=DEV, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ fits against the Newton oracle
@pytest.fixture(scope="module")
def optima():
    with np.load(os.path.join(GOLDEN, "softmax_reg_optima.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("tol", [1e-4, 1e-6])
@pytest.mark.parametrize("ci", range(6), ids=["C1e-7", "C1e-4", "C1e-2", "C1", "C1e2", "C1e7"])
@pytest.mark.parametrize("pi", range(3), ids=["3x4x3", "20x16x5", "130x68x33"])
def test_fit_reaches_the_oracles_minimiser(optima, pi, ci, tol):
    from mvlpt_amd.linear_probe import SoftmaxRegression
    N, D, K = (int(v) for v in optima["problems"][pi])
    X, y, Cw = optima[f"X{pi}"], optima[f"y{pi}"], float(optima["Cs"][ci])
    ts, mu = optima[f"theta{pi}_{ci}"], float(optima[f"mu{pi}_{ci}"])
    l2 = 1.0 / (Cw * N)
    clf = SoftmaxRegression(C=Cw, tol=tol, max_iter=1000, device=DEV).fit(X, y)
    th = np.concatenate([clf.coef_.ravel(), clf.intercept_]).astype(np.float64)
    g = R.gradient(th, X, y, K, l2)
    gb = R.eval_bounds(th, X, y, K, l2)["grad"].max()
    gap, gn = R.objective(th, X, y, K, l2) - R.objective(ts, X, y, K, l2), np.linalg.norm(g)
    dp = 16 * 2.0 ** -53 * max(1.0, abs(R.objective(ts, X, y, K, l2)))      # the two float64 objectives' own rounding
    print(f"N {N} C {Cw:g} tol {tol:g}: {clf.status_} after {clf.n_iter_}; max|g| {np.abs(g).max():.2e} <= {tol + gb:.2e}; "
          f"F - F* {gap:.2e} <= {gn * gn / mu:.2e}; |theta - theta*| {np.linalg.norm(th - ts):.2e} <= {2 * gn / mu:.2e}")
    assert clf.status_ == "gtol" and clf.converged_ and clf.n_iter_ < 1000
    assert np.abs(g).max() <= tol + gb
    assert -dp <= gap <= gn * gn / mu + dp
    if Cw <= 1:
        assert np.linalg.norm(th - ts) <= 2 * gn / mu
    assert abs(clf.intercept_.astype(np.float64).mean()) <= 1e-6 * max(1.0, np.abs(clf.intercept_).max())
    assert np.array_equal(clf.classes_, np.arange(K))
