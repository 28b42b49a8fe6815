"""Float64 oracle of the Tip-Adapter head (numpy only) and the error bounds of the device entries (mvlpt_op_tip_*).

With F [N, D] unit image features, K [NK, D] keys sorted by class, key_ptr [C + 1], W [C, D] unit text features:

    a_nj = <f_n, k_j>,  t_nj = beta (1 - a_nj),  A_nj = exp(-t_nj),
    z_nc = s <f_n, w_c> + alpha sum_{j in c} A_nj,
    loss = mean_n [logsumexp(z_n) - z_n[y_n]],  R = (softmax(z) - onehot) / N,
    dK_jd = alpha beta sum_n A_nj R_n,cls(j) f_nd.

Error bounds from float64 magnitudes (u = 2^-24), as tests/softmax_reg_ref.py derives its own:
    |da_nj|    <= (D + 1) u sum_d |f_nd| |k_jd|
    |dA_nj|    <= A_nj (beta |da_nj| + (2 |t_nj| + 4) u)                      product, argument scaling, exponential
    |dclip_nc| <= s (D + 2) u sum_d |f_nd| |w_cd|
    |dz_nc|    <= |dclip_nc| + alpha (sum_{j in c} |dA_nj| + (n_c + 1) u sum_{j in c} A_nj) + 2 u |z_nc|
    |dloss|    <= 2 max_nc |dz_nc| + 64 * 2^-53 (|loss| + 1) + u |loss|
    |dR_nc|    <= (2 p_nc max_c |dz_nc| + u |r_nc|) / N + 2^-149             (r = N R)
    |d dK_jd|  <= alpha beta [sum_n (|dA_nj| |R_n,cls(j)| + A_nj |dR_n,cls(j)|) |f_nd| + (N + 3) u sum_n A_nj |R_n,cls(j)| |f_nd|
                              + sum_n 2^-149 |f_nd|] + 2^-149
Three terms are not in the issue's list; each is a rounding step of the implementation:
    u |loss|          loss [1] is an fp32 output: the double sum is rounded once when it is stored.
    2^-149 in dR      R is stored in fp32; below 2^-126 that rounding is absolute, one subnormal spacing (softmax_reg_ref.TINY).
    2^-149 in d dK    the staged factor A R is an fp32 product of a number <= 1 with R: below 2^-126 it rounds absolutely too, once per
                      (n, j), and so does the stored dK.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
SCALE = 100.0      # exp(logit_scale) of a trained CLIP


SIGMA = 2.5
# (N, D, key counts per class): a single row; an empty class and a class wider than a key tile; ragged D and more classes than a class
# tile; the widths of the towers
HEAD_CASES = [(1, 64, (1, 1)), (96, 64, (1, 3, 16, 0, 2, 5, 130, 4)), (133, 68, (2,) * 130 + (1,)), (257, 512, (16,) * 37),
              (129, 640, (4,) * 100), (64, 1024, (1,) * 7)]
HEAD_HPARAMS = [(1.0, 5.5), (3.0, 7.0), (0.1, 0.1), (1.0, 0.0)]      # (alpha, beta)
SEARCH_CASES = [(96, 64, (1, 3, 16, 0, 2, 5, 130, 4)), (257, 68, (2,) * 130 + (1,)), (2000, 64, (1, 3, 16, 0, 2, 5, 130, 4))]
SEARCH_BETAS = (0.1, 0.5, 1.0, 2.0, 3.55, 5.5, 7.0)
SEARCH_ALPHAS = (0.1, 0.5, 1.0, 1.55, 3.0)
# the search of tests/test_hip_tip_adapter.py (the width of the test-size towers, a 7 x 5 grid of the published formula): noisier than
# the cases above, and drawn so that ONE grid point is best by more than twice the undecided rows (tests/test_tip_ref.py asserts it)
WINNER_CASE, WINNER_SIGMA, WINNER_SEED, WINNER_STEP = (200, 128, (1, 3, 16, 0, 2, 5, 130, 4)), 6.0, 3, (7, 5)


def case_seed(N, D, counts):
    return 1000 * N + D + len(counts)


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def make_case(N, D, counts, sigma, seed):
    """The generator of the tests: class prototypes are C random unit vectors, a key or a test feature is
    unit(proto[class] + sigma unit(noise)), W = unit(proto + 0.3 unit(noise)), labels uniform.  Everything fp32 (the device's inputs);
    the keys come sorted by class.  dict(F, y, K, key_ptr, key_cls, W)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    C = len(counts)
    proto = unit(rng.standard_normal((C, D)))
    key_cls = np.repeat(np.arange(C), counts)
    K = unit(proto[key_cls] + sigma * unit(rng.standard_normal((len(key_cls), D))))
    y = rng.integers(0, C, N)
    F = unit(proto[y] + sigma * unit(rng.standard_normal((N, D))))
    W = unit(proto + 0.3 * unit(rng.standard_normal((C, D))))
    key_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return {"F": F.astype(np.float32), "y": y.astype(np.int32), "K": K.astype(np.float32), "key_ptr": key_ptr,
            "key_cls": key_cls.astype(np.int64), "W": W.astype(np.float32)}


def key_table(labels, n_cls):
    """(stable order by class, key_ptr int32 [n_cls + 1]) of arbitrary key labels."""
    labels = np.asarray(labels, np.int64)
    order = np.argsort(labels, kind="stable")
    return order, np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=n_cls))]).astype(np.int32)


def seg_sum(X, key_ptr):
    """[N, NK] -> [N, C]: the sum of each class's columns; an empty class gives 0."""
    X = np.asarray(X, np.float64)
    out = np.zeros((X.shape[0], len(key_ptr) - 1))
    for c in range(len(key_ptr) - 1):
        if key_ptr[c + 1] > key_ptr[c]:
            out[:, c] = X[:, key_ptr[c]:key_ptr[c + 1]].sum(1)
    return out


def affinity(F, K, beta):
    a = np.asarray(F, np.float64) @ np.asarray(K, np.float64).T
    return np.exp(-beta * (1.0 - a))


def clip_logits(F, W, s=SCALE):
    return s * (np.asarray(F, np.float64) @ np.asarray(W, np.float64).T)


def logits(F, K, key_ptr, W, alpha, beta, s=SCALE):
    return clip_logits(F, W, s) + alpha * seg_sum(affinity(F, K, beta), key_ptr)


def softmax_stats(z, y):
    """(loss, p [N, C], R = (p - onehot) / N)."""
    N = z.shape[0]
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    p = np.exp(z - lse[:, None])
    R = p.copy()
    R[np.arange(N), y] -= 1.0
    return float(np.mean(lse - z[np.arange(N), y])), p, R / N


def train(F, y, K, key_ptr, key_cls, W, alpha, beta, s=SCALE):
    """dict(z, loss, R, dK, A) in float64."""
    A = affinity(F, K, beta)
    z = clip_logits(F, W, s) + alpha * seg_sum(A, key_ptr)
    loss, p, R = softmax_stats(z, np.asarray(y, np.int64))
    G = A * R[:, key_cls]                                   # [N, NK]
    dK = alpha * beta * (G.T @ np.asarray(F, np.float64))
    return {"z": z, "loss": loss, "p": p, "R": R, "dK": dK, "A": A}


# ---------------------------------------------------------------------------------------------- bounds of the device entries
def affinity_bound(F, K, beta):
    """(A, |dA|) [N, NK]."""
    F64, K64 = np.asarray(F, np.float64), np.asarray(K, np.float64)
    D = F64.shape[1]
    a = F64 @ K64.T
    t = beta * (1.0 - a)
    A = np.exp(-t)
    da = (D + 1) * U * (np.abs(F64) @ np.abs(K64).T)
    return A, A * (beta * da + (2.0 * np.abs(t) + 4.0) * U)


def clip_bound(F, W, s=SCALE):
    D = np.asarray(F).shape[1]
    return s * (D + 2) * U * (np.abs(np.asarray(F, np.float64)) @ np.abs(np.asarray(W, np.float64)).T)


def cache_bound(F, K, key_ptr, beta):
    """(cache [N, C], its bound per unit of alpha [N, C])."""
    A, dA = affinity_bound(F, K, beta)
    n_c = np.diff(np.asarray(key_ptr, np.int64))
    cache = seg_sum(A, key_ptr)
    return cache, seg_sum(dA, key_ptr) + (n_c + 1)[None, :] * U * cache


def logits_bound(F, K, key_ptr, W, alpha, beta, s=SCALE):
    """(z, |dz|) [N, C]."""
    cache, dcache = cache_bound(F, K, key_ptr, beta)
    z = clip_logits(F, W, s) + alpha * cache
    return z, clip_bound(F, W, s) + abs(alpha) * dcache + 2.0 * U * np.abs(z)


def train_bounds(F, y, K, key_ptr, key_cls, W, alpha, beta, s=SCALE):
    """dict of the bounds in the module docstring: z, loss, R, dK; and ref, the float64 results."""
    ref = train(F, y, K, key_ptr, key_cls, W, alpha, beta, s)
    F64 = np.asarray(F, np.float64)
    N = F64.shape[0]
    A, dA = affinity_bound(F, K, beta)
    _, dz = logits_bound(F, K, key_ptr, W, alpha, beta, s)
    dzmax = dz.max(1)
    dloss = 2.0 * dzmax.max() + 64 * 2.0 ** -53 * (abs(ref["loss"]) + 1.0) + U * abs(ref["loss"])
    r = ref["R"] * N
    dR = (2.0 * ref["p"] * dzmax[:, None] + U * np.abs(r)) / N + TINY
    Ra, Fa = np.abs(ref["R"])[:, key_cls], np.abs(F64)
    ddK = abs(alpha * beta) * ((dA * Ra + A * dR[:, key_cls]).T @ Fa + (N + 3) * U * ((A * Ra).T @ Fa) + TINY * Fa.sum(0)[None, :]) + TINY
    return {"z": dz, "loss": dloss, "R": dR, "dK": ddK, "ref": ref}


def decided(z, dz):
    """Rows whose float64 top-1 minus top-2 margin exceeds 2 max_c |dz|: every evaluation inside the bound has the same arg-max."""
    if z.shape[1] == 1:
        return np.ones(z.shape[0], bool)
    top = np.sort(z, 1)
    return (top[:, -1] - top[:, -2]) > 2.0 * dz.max(1)


def published_grid(scale=(7.0, 3.0), step=(200, 20)):
    """The grid of the published search: beta_i = i (scale[0] - 0.1) / step[0] + 0.1, alpha_j likewise."""
    betas = [i * (scale[0] - 0.1) / step[0] + 0.1 for i in range(step[0])]
    alphas = [i * (scale[1] - 0.1) / step[1] + 0.1 for i in range(step[1])]
    return np.asarray(betas, np.float64), np.asarray(alphas, np.float64)


def search(F, y, K, key_ptr, W, betas, alphas, s=SCALE):
    """dict(counts, sure, undecided) int64 [nb, na] from the float64 reference: counts of the reference's own arg-max, the decided rows
    that are correct, and the rows that are not decided.  betas / alphas: the fp32 values the device gets."""
    y = np.asarray(y, np.int64)
    nb, na = len(betas), len(alphas)
    clip, dclip = clip_logits(F, W, s), clip_bound(F, W, s)
    out = {k: np.zeros((nb, na), np.int64) for k in ("counts", "sure", "undecided")}
    for b, beta in enumerate(betas):
        cache, dcache = cache_bound(F, K, key_ptr, float(beta))
        for a, alpha in enumerate(alphas):
            z = clip + float(alpha) * cache
            ok = decided(z, dclip + abs(float(alpha)) * dcache + 2.0 * U * np.abs(z))
            hit = z.argmax(1) == y
            out["counts"][b, a] = hit.sum()
            out["sure"][b, a] = (hit & ok).sum()
            out["undecided"][b, a] = (~ok).sum()
    return out


def winner(counts):
    """The published loop updates only on `>`: the first strict maximum in beta-major order.  (b, a)."""
    counts = np.asarray(counts)
    flat = int(np.argmax(counts.ravel()))      # numpy's arg-max is the first maximum
    return flat // counts.shape[1], flat % counts.shape[1]


def adamw_step(p, g, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01):
    """The first AdamW step from zero moments, float64."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    m, v = (1 - beta1) * g, (1 - beta2) * g * g
    mh, vh = m / (1 - beta1), v / (1 - beta2)
    return p * (1 - lr * weight_decay) - lr * mh / (np.sqrt(vh) + eps)
