"""Float64 oracle of the softmax-regression objective behind the linear probe (numpy only: the GPU box may lack sklearn).

    F(W, b) = (1/N) sum_i [logsumexp(z_i) - z_i[y_i]] + (l2/2) |W|_F^2,   z_i = W x_i + b,   l2 = 1 / (C N),   b unpenalised

is what sklearn 1.7's LogisticRegression(solver="lbfgs", penalty="l2", C=C) minimises (tests/test_softmax_reg_ref.py pins that on
recorded sklearn solutions).  theta = [W row-major [K, D] | b [K]], the layout of the device entries.

F is invariant under b + c 1, so the Hessian has the null direction v = (0, 1_K) / sqrt(K) and the minimiser is unique only up to it:
`newton` returns the one with centred intercepts, and `mu` is the smallest Hessian eigenvalue on the complement of v.

Error bounds of the device evaluation, from float64 magnitudes (u = 2^-24):
    |dz_ik|  <= (D + 2) u (sum_j |x_ij| |w_kj| + |b_k|)                 a D-term fp32 fma chain, the bias add, one store
    |dF|     <= max_i 2 max_k |dz_ik| + 64 * 2^-53 * (|F| + 1)            log-sum-exp is 1-Lipschitz in max norm, minus z_y
    |dR_ik|  <= (2 p_ik max_k |dz_ik| + u |r_ik|) / N + 2^-149            softmax moves by at most 2 p |dz|_max; one fp32 rounding
                                                                          (relative, or one subnormal spacing where R underflows)
    |dG_kd|  <= sum_i |dR_ik| |x_id| + (N + 2) u sum_i |r_ik| |x_id| + u l2 |w_kd|
(r_ik = N R_ik; the issue states |dR| with r in that unit, we keep it).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149      # spacing of the fp32 subnormals: the rounding of an R below 2^-126 is absolute, not relative


def split(theta, K, D):
    theta = np.asarray(theta, np.float64)
    return theta[:K * D].reshape(K, D), theta[K * D:]


def probs(theta, X, K):
    """(z, p, lse) in float64."""
    X = np.asarray(X, np.float64)
    W, b = split(theta, K, X.shape[1])
    z = X @ W.T + b
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    return z, np.exp(z - lse[:, None]), lse


def objective(theta, X, y, K, l2):
    W, _ = split(theta, K, X.shape[1])
    z, _, lse = probs(theta, X, K)
    return float(np.mean(lse - z[np.arange(len(y)), y]) + 0.5 * l2 * np.sum(W * W))


def gradient(theta, X, y, K, l2):
    X = np.asarray(X, np.float64)
    N, D = X.shape
    W, _ = split(theta, K, D)
    _, p, _ = probs(theta, X, K)
    R = p.copy()
    R[np.arange(N), y] -= 1.0
    R /= N
    return np.concatenate([(R.T @ X + l2 * W).ravel(), R.sum(0)])


def hessian(theta, X, K, l2):
    """The exact Hessian [n, n], n = K D + K, in theta's layout."""
    X = np.asarray(X, np.float64)
    N, D = X.shape
    _, p, _ = probs(theta, X, K)
    Xa = np.concatenate([X, np.ones((N, 1))], 1)                     # [N, D + 1]
    H4 = np.empty((K, D + 1, K, D + 1))
    for k in range(K):
        M = -p[:, k:k + 1] * p                                        # [N, K]: p_ik (delta_kl - p_il)
        M[:, k] += p[:, k]
        A = (Xa[:, None, :] * M[:, :, None]).reshape(N, K * (D + 1))  # [N, (l, b)]
        H4[k] = (Xa.T @ A).reshape(D + 1, K, D + 1) / N
    n = K * D + K
    # (k, a) of the augmented layout -> position in [W | b]
    pos = np.empty((K, D + 1), np.int64)
    pos[:, :D] = np.arange(K * D).reshape(K, D)
    pos[:, D] = K * D + np.arange(K)
    H = np.empty((n, n))
    H[np.ix_(pos.ravel(), pos.ravel())] = H4.reshape(K * (D + 1), K * (D + 1))
    H[np.arange(K * D), np.arange(K * D)] += l2
    return H


def null_direction(K, D):
    v = np.zeros(K * D + K)
    v[K * D:] = 1.0 / np.sqrt(K)
    return v


def centre(theta, K, D):
    theta = np.array(theta, np.float64)
    theta[K * D:] -= theta[K * D:].mean()
    return theta


def newton(X, y, K, l2, gtol=1e-13, max_iter=200):
    """The minimiser (centred intercepts) by damped Newton steps from zero: the step solves (H + s v v^T) d = -g, which is the
    pseudo-inverse step because g is orthogonal to the null direction v; halving until F does not increase."""
    X = np.asarray(X, np.float64)
    N, D = X.shape
    n = K * D + K
    v = null_direction(K, D)
    theta = np.zeros(n)
    f = objective(theta, X, y, K, l2)
    for _ in range(max_iter):
        g = gradient(theta, X, y, K, l2)
        if np.abs(g).max() < gtol:
            break
        H = hessian(theta, X, K, l2)
        s = max(float(np.diag(H).max()), 1e-300)
        d = -np.linalg.solve(H + s * np.outer(v, v), g)
        t = 1.0
        while True:
            cand = theta + t * d
            fc = objective(cand, X, y, K, l2)
            # close to the optimum the decrease of F drops under its rounding: there a step that halves the gradient is taken
            if fc <= f or t < 1e-12 or np.abs(gradient(cand, X, y, K, l2)).max() < 0.5 * np.abs(g).max():
                break
            t *= 0.5
        theta, f = centre(cand, K, D), fc
    g = gradient(theta, X, y, K, l2)
    assert np.abs(g).max() < gtol, f"Newton stopped at max|grad| {np.abs(g).max():.3e}"
    return theta


def mu(theta, X, K, l2):
    """The smallest eigenvalue of the Hessian at theta on the complement of the intercept null direction."""
    D = np.asarray(X).shape[1]
    H = hessian(theta, X, K, l2)
    v = null_direction(K, D)
    s = float(np.diag(H).max())
    return float(np.linalg.eigvalsh(H + s * np.outer(v, v))[0])


# ---------------------------------------------------------------------------------------------- bounds of the device evaluation
def logit_bound(theta, X, K):
    X = np.asarray(X, np.float64)
    W, b = split(theta, K, X.shape[1])
    return (X.shape[1] + 2) * U * (np.abs(X) @ np.abs(W).T + np.abs(b))      # [N, K]


def eval_bounds(theta, X, y, K, l2):
    """dict of the bounds in the module docstring: z [N, K], F, R [N, K], grad [K D + K]."""
    X = np.asarray(X, np.float64)
    N, D = X.shape
    W, _ = split(theta, K, D)
    _, p, _ = probs(theta, X, K)
    dz = logit_bound(theta, X, K)
    dzmax = dz.max(1)
    r = p.copy()
    r[np.arange(N), y] -= 1.0
    F = objective(theta, X, y, K, l2)
    dF = 2.0 * dzmax.max() + 64 * 2.0 ** -53 * (abs(F) + 1.0)
    dR = (2.0 * p * dzmax[:, None] + U * np.abs(r)) / N + TINY
    Ra = np.abs(r) / N
    Xa = np.abs(X)
    dGW = dR.T @ Xa + (N + 2) * U * (Ra.T @ Xa) + U * l2 * np.abs(W)
    dGb = dR.sum(0) + (N + 2) * U * Ra.sum(0)
    return {"z": dz, "F": dF, "R": dR, "grad": np.concatenate([dGW.ravel(), dGb])}


def make_problem(N, D, K, seed, spread=1.0):
    """Gaussian class blobs: X fp32 [N, D], y int64 [N] with every class present when N >= K."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, D))
    y = np.arange(N) % K
    rng.shuffle(y)
    X = (centres[y] + spread * rng.standard_normal((N, D))).astype(np.float32)
    return X, y.astype(np.int64)


def eval_fp32(theta, X, y, K, l2, direction=None):
    """A numpy restatement of the device evaluation's precision: fp32 logits, the row stage in float64, R rounded once to fp32, an
    fp32 gradient product.  (grad float32 [K D + K], [F, max|g|, g.dir, |g|^2]).  Not bit-equal to the device: same error classes."""
    X = np.asarray(X, np.float32)
    N, D = X.shape
    theta = np.asarray(theta, np.float32)
    W, b = theta[:K * D].reshape(K, D), theta[K * D:]
    z = (X @ W.T + b).astype(np.float64)
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    R = np.exp(z - lse[:, None])
    R[np.arange(N), y] -= 1.0
    R = (R / N).astype(np.float32)
    F = float(np.sum(lse - z[np.arange(N), y]) / N + 0.5 * l2 * np.sum(W.astype(np.float64) ** 2))
    gW = ((R.T @ X).astype(np.float64) + l2 * W.astype(np.float64)).astype(np.float32)
    g = np.concatenate([gW.ravel(), R.astype(np.float64).sum(0).astype(np.float32)])
    g64 = g.astype(np.float64)
    gd = float(g64 @ np.asarray(direction, np.float64)) if direction is not None else 0.0
    return g, [F, float(np.abs(g64).max()), gd, float(g64 @ g64)]
