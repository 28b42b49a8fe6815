"""TEST INFRASTRUCTURE — float64 oracle, derived tolerance and inputs of the nearest-token tests (tests/test_hip_nearest.py,
tests/test_interpret_host.py).

Tolerance of one distance, derived, not measured: a term (q_i - e_i)^2 carries at most 3 roundings, a sum of d non-negative terms in
any order adds (d - 1) u, the square root halves the relative error and adds one rounding:
    |dist - D64| <= (d / 2 + 3) * 2^-24 * D64,        and D64 == 0 must come out as exactly 0.0.
"""
from __future__ import annotations

import functools
import os

import numpy as np

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interpret.npz")


def tol(d: int) -> float:
    return (d / 2 + 3) * U


def dist64(Q: np.ndarray, E: np.ndarray) -> np.ndarray:
    """D64[r, t] = sqrt(sum_i (q_i - e_i)^2) in float64 from the fp32 inputs, difference form (blocks of table rows that stay in cache)."""
    Q64 = Q.astype(np.float64)
    out = np.empty((Q.shape[0], E.shape[0]), dtype=np.float64)
    step = max(1, (1 << 19) // E.shape[1])
    for t0 in range(0, E.shape[0], step):
        E64 = E[t0:t0 + step].astype(np.float64)
        for r in range(Q.shape[0]):
            diff = E64 - Q64[r]
            out[r, t0:t0 + step] = np.einsum("ij,ij->i", diff, diff)
    return np.sqrt(out, out=out)


def topk64(D: np.ndarray, k: int) -> np.ndarray:
    """argsort[:k] by (distance, index): a stable sort on the distance keeps the smaller index first."""
    return np.argsort(D, axis=1, kind="stable")[:, :k]


def plant(E: np.ndarray, Q: np.ndarray, k: int, rng: np.random.Generator) -> np.ndarray:
    """Overwrite n = min(k + 1, V) distinct rows of E per query with fp32(Q[r] + 1e-4 (1 + j / 4) v_j), v_j a random unit vector,
    j = 0 .. n-1; returns the ids [R, n].  Consecutive planted neighbours are then >= 1.4e-2 apart relatively (j + 1 = 65: 17.25 / 17),
    hundreds of tolerances, while random neighbours alone can be 1.5e-6 apart."""
    V, d = E.shape
    R = Q.shape[0]
    n = min(k + 1, V)
    assert R * n <= V
    ids = rng.permutation(V)[:R * n].reshape(R, n)
    v = rng.standard_normal((R, n, d))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    for j in range(n):
        E[ids[:, j]] = (Q.astype(np.float64) + 1e-4 * (1 + j / 4) * v[:, j]).astype(np.float32)
    return ids


@functools.lru_cache(maxsize=None)
def inputs(seed: int, V: int, d: int, R: int, k: int, planted: bool = True):
    """(Q fp32 [R, d], E fp32 [V, d], planted ids or None, D64 [R, V]): drawn once per shape, shared, never written to."""
    rng = np.random.default_rng(seed)
    E = (0.02 * rng.standard_normal((V, d))).astype(np.float32)
    Q = (0.02 * rng.standard_normal((R, d))).astype(np.float32)
    ids = plant(E, Q, k, rng) if planted else None
    D = dist64(Q, E)
    for a in (Q, E, D):
        a.setflags(write=False)
    return Q, E, ids, D


def assert_separated(D: np.ndarray, ids: np.ndarray, k: int, d: int) -> np.ndarray:
    """On the oracle alone: the float64 top-k is the planted ids in order and consecutive neighbours (the (k+1)-th included, when
    there is one) are more than 8 tolerances apart.  Returns the float64 top-k."""
    n = min(k + 1, D.shape[1])
    want = topk64(D, n)
    assert np.array_equal(want, ids[:, :n]), "the float64 neighbours are not the planted rows"
    s = np.take_along_axis(D, want, axis=1)
    if n > 1:
        gap = (s[:, 1:] - s[:, :-1]) / s[:, 1:]
        assert gap.min() > 8 * tol(d), f"smallest relative gap {gap.min():.3e} against tolerance {tol(d):.3e}"
    return want[:, :k]


def assert_dist_inside(dist: np.ndarray, want64: np.ndarray, d: int, what: str = "dist") -> float:
    """|dist - D64| <= tol * D64 elementwise, exactly 0.0 where D64 == 0; returns the worst error in units of the bound."""
    dist = np.asarray(dist, dtype=np.float64)
    err = np.abs(dist - want64)
    bound = tol(d) * want64
    assert np.all(err <= bound), f"{what}: worst |err| / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3f}"
    assert np.all(dist[want64 == 0] == 0.0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def golden_table(fix) -> np.ndarray:
    """The fixture's planted table: mvlpt_amd.weights._randn("token_embedding.weight", seed, [vocab, width], 0.02), as FrozenCLIP falls
    back to and make_state_dict(include_token_embedding=True) builds, with the stored planted rows written over the stored ids."""
    from mvlpt_amd.weights import _randn
    E = _randn("token_embedding.weight", int(fix["table_seed"]), (int(fix["vocab"]), int(fix["width"])), 0.02).numpy().copy()
    E[fix["planted_ids"].reshape(-1)] = fix["planted_rows"].reshape(-1, E.shape[1])
    return E
