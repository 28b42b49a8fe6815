"""Evaluation kernels on the device (-m gpu): mvlpt_op_eval_count and mvlpt_op_eval_rank_columns against numpy.

There is no tolerance anywhere but one: the counters are integers and compared with array_equal, the rank statistics are compared
exactly with the numpy emulation of the same integer formulation (mvlpt_amd.evaluator.rank_statistics_numpy, itself shown equal to
metrics.py by tests/test_eval_host.py), and the finished metrics with `==` against mvlpt_amd/metrics.py.  Only the recorded reference
values of tests/golden/metrics.npz are met at the 1e-12 that tests/test_metrics.py uses for the host functions."""
import numpy as np
import pytest
import torch

from mvlpt_amd import evaluator as E
from mvlpt_amd import metrics as M
from tests.golden_util import load_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = 4096                                                                 # MVLPT_EVAL_SORT_TILE (asserted below)
PAD = 7                                                                  # the logits are a column slice: pitch C + PAD


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ counters
def batch(rng, B, C, variant):
    """logits [B, C] with ties everywhere (8 values), labels and task ids; row 0 carries the variant's special case"""
    x = rng.integers(0, 8, (B, C)).astype(np.float32)
    for r in range(min(B, 3)):
        kind = (variant + r) % 3
        if kind == 0:
            x[r, 0] = x[r, C - 1] = 9.0                                  # the maximum tied between the first and the last column
        elif kind == 1:
            x[r, C - 1] = 9.0                                            # the maximum in the last column
        else:
            x[r, C // 2] = np.nan                                        # a NaN counts as maximal, the first one wins
            x[r, C - 1] = np.nan
    return x, rng.integers(0, C, B).astype(np.int64), rng.integers(0, 3, B).astype(np.int32)


def reference(x, y, task, lo, hi, C, mask=None):
    keep = np.ones(C, bool) if mask is None else mask.astype(bool)
    idx = np.nonzero(keep)[0]
    pred = idx[np.argmax(x[:, idx], axis=1)]
    pred_r = np.array([max(lo[t], 0) + np.argmax(x[r, lo[t]:hi[t]]) for r, t in enumerate(task)], dtype=np.int64)
    out = {"n_true": np.bincount(y, minlength=C), "n_pred": np.bincount(pred, minlength=C),
           "n_hit": np.bincount(y[pred == y], minlength=C), "n_pred_r": np.bincount(pred_r, minlength=C),
           "n_hit_r": np.bincount(y[pred_r == y], minlength=C), "cmat": np.zeros((C, C), np.int64)}
    np.add.at(out["cmat"], (y, pred), 1)
    return out


@pytest.mark.parametrize("B", [1, 100])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 1000, 2191])
def test_counters_accumulate_exactly(C, B):
    from mvlpt_amd.engine import op_eval_count
    rng = np.random.default_rng(C * 1000 + B)
    lo, hi = np.array([0, 0, C // 2], np.int32), np.array([1, C, C], np.int32)        # widths 1, full, upper half
    calls = [batch(rng, B, C, v) for v in range(3)]
    X, Y, TK = (np.concatenate([c[i] for c in calls]) for i in range(3))
    want = reference(X, Y, TK, lo, hi, C)
    for with_cmat, onehot in ((True, False), (False, True)):
        buf = torch.zeros(5 * C + C * C, device=DEV, dtype=torch.int64)
        v = {k: buf[i * C:(i + 1) * C] for i, k in enumerate(("n_true", "n_pred", "n_hit", "n_pred_r", "n_hit_r"))}
        for x, y, tk in calls:
            wide = torch.full((B, C + PAD), 99.0, device=DEV)            # a larger value outside the slice must never be seen
            wide[:, 3:3 + C] = dev(x)
            labels = dev(np.eye(C, dtype=np.float32)[y]) if onehot else dev(y)
            op_eval_count(wide[:, 3:3 + C], labels, v["n_true"], v["n_pred"], v["n_hit"], task=dev(tk), lo=dev(lo), hi=dev(hi),
                          n_pred_r=v["n_pred_r"], n_hit_r=v["n_hit_r"], cmat=buf[5 * C:] if with_cmat else None)
        got = buf.cpu().numpy()
        for i, k in enumerate(("n_true", "n_pred", "n_hit", "n_pred_r", "n_hit_r")):
            assert np.array_equal(got[i * C:(i + 1) * C], want[k]), (k, with_cmat, onehot)
        assert np.array_equal(got[5 * C:].reshape(C, C), want["cmat"] if with_cmat else np.zeros((C, C), np.int64))


@pytest.mark.parametrize("C", [2, 65, 1000])
def test_column_mask_row_list_and_column_occurrence(C):
    from mvlpt_amd.engine import op_eval_count
    rng = np.random.default_rng(C)
    B = 100
    x, _, _ = batch(rng, B, C, 0)
    tgt = (rng.random((B, C)) < 0.02).astype(np.float32)
    tgt[:, C - 1] = 0.0                                                  # a column that never occurs ...
    x[:, C - 1] = 50.0                                                   # ... and would win every unmasked arg-max
    tgt[np.arange(B), rng.integers(0, C - 1, B)] = 1.0
    tgt[6] = 0.0                                                         # a row without a target: arg-max of zeros, the first kept column
    rows = np.arange(0, B, 3).astype(np.int32)
    seen = torch.zeros(C, device=DEV, dtype=torch.uint8)
    buf = torch.zeros(3 * C, device=DEV, dtype=torch.int64)
    n_true, n_pred, n_hit = buf[:C], buf[C:2 * C], buf[2 * C:]
    op_eval_count(dev(x), dev(tgt), n_true, n_pred, n_hit, rows=dev(rows), col_seen=seen)
    keep = np.any(tgt[rows] != 0, axis=0)
    assert np.array_equal(seen.cpu().numpy().astype(bool), keep) and not keep[C - 1]
    buf.zero_()
    op_eval_count(dev(x), dev(tgt), n_true, n_pred, n_hit, rows=dev(rows), col_mask=seen)
    idx = np.nonzero(keep)[0]
    t, p = idx[np.argmax(tgt[rows][:, idx], axis=1)], idx[np.argmax(x[rows][:, idx], axis=1)]
    got = buf.cpu().numpy()
    assert np.array_equal(got[:C], np.bincount(t, minlength=C))
    assert np.array_equal(got[C:2 * C], np.bincount(p, minlength=C))
    assert np.array_equal(got[2 * C:], np.bincount(t[t == p], minlength=C))
    fn = E.device_metric("mean-per-class")
    assert fn(dev(tgt), dev(x), rows=dev(rows)) == M.balanced_accuracy_score(tgt[rows], x[rows])


# ------------------------------------------------------------------------------------------------ rank columns
KINDS = ["continuous", "quantised", "equal", "zeros", "fp16"]
WIDE = 5 + 65 + 3


def scores(rng, kind, N):
    s = rng.standard_normal((N, WIDE)).astype(np.float32)
    if kind == "quantised":
        s = rng.integers(0, 4, (N, WIDE)).astype(np.float32)            # 4 values: runs of ties far longer than a tile
    elif kind == "equal":
        s[:] = 0.25
    elif kind == "zeros":
        s = rng.choice(np.array([0.0, -0.0, 1.0], dtype=np.float32), (N, WIDE))
    elif kind == "fp16":
        s = s.astype(np.float16).astype(np.float32)
    return s


def targets(rng, N):
    """a 0/1 matrix whose slice columns 0, 1, 2 hold 0, exactly 1 and N positives; int labels in [0, 3) for the other form"""
    t = (rng.random((N, WIDE)) < 0.3).astype(np.float32)
    t[:, 5], t[:, 6], t[:, 7] = 0.0, 0.0, 1.0
    t[rng.integers(0, N), 6] = 1.0
    return t, rng.integers(0, 3, N).astype(np.int64)


def outcome(fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except ValueError as e:
        return ("ValueError", str(e))


def check_rank(s, tm, y, C, rows):
    from mvlpt_amd.engine import op_eval_rank_columns
    sel = np.arange(len(s)) if rows is None else rows
    rows_d = None if rows is None else dev(rows.astype(np.int32))
    sd, td = dev(s), dev(tm)
    for form in ("matrix", "labels"):
        tgt = td[:, 5:5 + C] if form == "matrix" else dev(y)
        out = op_eval_rank_columns(sd[:, 5:5 + C], tgt, rows=rows_d)
        again = op_eval_rank_columns(sd[:, 5:5 + C], tgt, rows=rows_d)
        assert torch.equal(out["packed"], again["packed"])               # two calls give equal bits
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for c in range(C):
            positive = tm[sel, 5 + c] == 1 if form == "matrix" else y[sel] == c
            n_pos, n_neg, twice_u, interp = E.rank_statistics_numpy(s[sel, 5 + c], positive)
            assert (got["n_pos"][c], got["n_neg"][c], got["twice_u"][c]) == (n_pos, n_neg, twice_u), (form, c)
            assert np.array_equal(got["interp"][c], interp), (form, c)
        assert not got["flags"].any()
    # the finished metrics, `==` against metrics.py, the same ValueError included
    yt, ys = tm[sel, 5:5 + C], s[sel, 5:5 + C]
    for name in ("11point_mAP", "roc_auc", "mean-per-class"):
        for lo in (5, 8):                                                # columns 5 .. 7 are degenerate: roc_auc raises there
            if lo + C > WIDE:
                continue
            got = outcome(E.device_metric(name), td[:, lo:lo + C], sd[:, lo:lo + C], rows=rows_d)
            want = outcome(M.get_metric(name), tm[sel, lo:lo + C], s[sel, lo:lo + C]) if len(sel) else 0.0
            if len(sel) == 0 and name == "roc_auc":
                continue                                                 # numpy's mean of nothing: not a case metrics.py defines
            assert got == want, (name, lo)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000, T, T + 1, 2 * T + 3])
def test_rank_columns_exact(N, kind):
    from mvlpt_amd import _lib
    assert _lib.EVAL_SORT_TILE == T
    rng = np.random.default_rng(N * 10 + KINDS.index(kind))
    s = scores(rng, kind, N)
    tm, y = targets(rng, N)
    # every N and kind meets every C, every row list and both target forms
    check_rank(s, tm, y, 1, None)
    check_rank(s, tm, y, 3, np.arange(0, N, 3))
    check_rank(s, tm, y, 3, None)
    check_rank(s, tm, y, 1, np.zeros(0, np.int64))
    check_rank(s, tm, y, 65, None if N % 2 else np.arange(0, N, 3))


def test_rank_columns_at_the_row_limit():
    """N = MVLPT_EVAL_MAX_ROWS: every stride of the network over the scratch buffer, sums beyond 2^32"""
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import eval_workspace_bytes, op_eval_rank_columns
    N = _lib.EVAL_MAX_ROWS
    rng = np.random.default_rng(20)
    s = np.stack([rng.standard_normal(N).astype(np.float32), rng.integers(0, 1000, N).astype(np.float32)], axis=1)
    y = rng.integers(0, 2, N).astype(np.int64)
    assert eval_workspace_bytes(N, 2) == 2 * N * 8 and eval_workspace_bytes(T, 2) == 0 and eval_workspace_bytes(T + 1, 2) == 2 * 2 * T * 8
    out = {k: v.cpu().numpy() for k, v in op_eval_rank_columns(dev(s), dev(y)).items()}
    for c in range(2):
        n_pos, n_neg, twice_u, interp = E.rank_statistics_numpy(s[:, c], y == c)
        assert (out["n_pos"][c], out["n_neg"][c], out["twice_u"][c]) == (n_pos, n_neg, twice_u) and twice_u > 2 ** 32
        assert np.array_equal(out["interp"][c], interp)
    assert not out["flags"].any()


def test_non_finite_scores_raise_the_flag_and_go_to_the_host():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import op_eval_rank_columns
    rng = np.random.default_rng(5)
    N, C = 300, 4
    s = rng.standard_normal((N, C)).astype(np.float32)
    s[7, 0], s[8, 1], s[9, 2], s[10, 2] = np.nan, np.inf, -np.inf, -np.inf
    y = rng.integers(0, C, N)
    oh = np.eye(C, dtype=np.float32)[y]
    out = op_eval_rank_columns(dev(s), dev(oh))
    assert out["flags"].cpu().tolist() == [_lib.EVAL_FLAG_NONFINITE] * 3 + [0]
    soft = oh.copy()
    soft[3, 3] = 0.5
    assert op_eval_rank_columns(dev(s), dev(soft))["flags"].cpu().tolist()[3] == _lib.EVAL_FLAG_SOFT_TARGET
    for name in ("11point_mAP", "roc_auc"):
        with np.errstate(all="ignore"):
            want = M.get_metric(name)(oh, s)
            got = E.device_metric(name)(dev(oh), dev(s))
        assert got == want or (np.isnan(got) and np.isnan(want))


def test_golden_cases_meet_the_recorded_reference_values():
    g = load_npz("metrics")
    tol = 1e-12                                                          # the bound of tests/test_metrics.py
    for i in g["cases"]:
        # the recorded scores are doubles; the device route takes the fp32 logits of the engine.  Every figure depends on the order
        # and the ties of the scores alone, and rounding these to fp32 merges no two of them (asserted), so the recorded values hold
        s, y, oh = g[f"c{i}_score"].astype(np.float32), g[f"c{i}_y"], g[f"c{i}_onehot"].astype(np.float32)
        for c in range(s.shape[1]):
            assert np.array_equal(np.argsort(s[:, c], kind="stable"), np.argsort(g[f"c{i}_score"][:, c], kind="stable"))
            assert len(np.unique(s[:, c])) == len(np.unique(g[f"c{i}_score"][:, c]))
        sd, yd, od = dev(s), dev(y.astype(np.int64)), dev(oh)
        assert abs(E.device_metric("accuracy")(yd, sd) - float(g[f"c{i}_accuracy"])) <= tol
        assert abs(E.device_metric("mean-per-class")(od, sd) - float(g[f"c{i}_mean_per_class"])) <= tol
        assert abs(E.device_metric("11point_mAP")(od, sd) - float(g[f"c{i}_map11"])) <= tol
        assert E.device_metric("11point_mAP")(yd, sd) == M.map_11_points(y, s)
        if f"c{i}_roc_auc" in g:
            assert abs(E.device_metric("roc_auc")(od, sd) - float(g[f"c{i}_roc_auc"])) <= tol
        else:
            with pytest.raises(ValueError, match="Only one class present"):
                E.device_metric("roc_auc")(od, sd)


def test_bad_arguments_are_refused_before_a_launch():
    import ctypes as C

    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    x = torch.zeros(4, 8, device=DEV)
    y = torch.zeros(4, device=DEV, dtype=torch.int64)
    cnt = torch.zeros(8, device=DEV, dtype=torch.int64)
    rc = _lib.lib.mvlpt_op_eval_count(_ptr(x), 4, 4, 8, _ptr(y), 0, 0, None, 0, None, None, None, 0, None, None, _ptr(cnt), _ptr(cnt),
                                      _ptr(cnt), None, None, None, _stream())
    assert rc == _lib.ERR_ARG and "pitch" in _lib.last_error(None)
    out = C.c_int64()
    assert _lib.lib.mvlpt_eval_workspace_bytes(_lib.EVAL_MAX_ROWS + 1, 1, _stream(), C.byref(out)) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.mvlpt_eval_workspace_bytes(0, 1, _stream(), C.byref(out)) == _lib.ERR_ARG
    assert torch.equal(cnt, torch.zeros_like(cnt))
