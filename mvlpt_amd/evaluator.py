"""Evaluation on the device (DESIGN.md scope row f1b): everything `MVLPT.test` reports is a function of integer counts, which the
two kernels of csrc/evaluate.hip produce exactly; this module finishes them on the host with the numpy calls `mvlpt_amd/metrics.py`
makes, so the values are bit-equal to the host route, not merely close.

* `DeviceClassification` — Dassl's `Classification` evaluator (`reset / process / evaluate`), which the reference's CoOp, CoCoOp and
  zero-shot trainers report through, plus the per-task ranged accuracy of trainers/mvlpt.py:1035-1039.  `process` is one launch of the
  streaming class counters and nothing else; `evaluate` reads the counters back once.  Dassl is not available here: its formulas
  (accuracy, error rate, `100 * f1_score(average="macro", labels=np.unique(y_true))`, the per-class table, the row-normalised
  `confusion_matrix(normalize="true")` saved to OUTPUT_DIR/cmat.pt) and its printed lines are RECALLED FROM UPSTREAM, as SURVEY.md
  Appendix B says of every Dassl behaviour; the sklearn parts are pinned by tests/golden/classification_eval.npz.
* `device_metric(name)` — the twin of `metrics.get_metric` for device tensors: accuracy, mean-per-class, 11point_mAP, roc_auc
  (trainers/vision_benchmark/datasets/metrics.py:1254-1294).

The finishing functions (`finish_*`, `classification_results`, `confusion_matrix`) take plain numpy count vectors and run anywhere."""
from __future__ import annotations

import os.path as osp
from collections import OrderedDict

import numpy as np

from . import metrics as M

ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


# ------------------------------------------------------------------------------------------------ finishing on the host (numpy only)
def classification_results(n_true, n_pred, n_hit, total=None) -> "OrderedDict[str, float]":
    """Dassl's three figures from per-class counts: truths, predictions and hits per label, `total` samples (default: sum of n_true)."""
    n_true, n_pred, n_hit = (np.asarray(v, dtype=np.int64) for v in (n_true, n_pred, n_hit))
    total = int(n_true.sum()) if total is None else int(total)
    correct = int(n_hit.sum())
    acc = 100.0 * correct / max(total, 1)
    occurs = np.nonzero(n_true)[0]                                       # labels=np.unique(y_true)
    # sklearn: f = (1 + beta^2) tp / (beta^2 true_sum + pred_sum) per label, macro = np.average(f)
    f1 = 2.0 * n_hit[occurs].astype(np.float64) / (n_true[occurs] + n_pred[occurs]).astype(np.float64)
    macro_f1 = 100.0 * float(np.average(f1)) if occurs.size else 0.0
    return OrderedDict(accuracy=acc, error_rate=100.0 - acc, macro_f1=macro_f1)


def perclass_table(n_true, n_hit, lab2cname=None):
    """[(label, classname, total, correct, acc %)] over the labels that occur, and their mean (Dassl's `perclass_accuracy`)."""
    rows = []
    for label in np.nonzero(np.asarray(n_true))[0].tolist():
        total, correct = int(n_true[label]), int(n_hit[label])
        name = lab2cname.get(label, str(label)) if lab2cname else str(label)
        rows.append((label, name, total, correct, 100.0 * correct / total))
    return rows, (float(np.mean([r[4] for r in rows])) if rows else 0.0)


def confusion_matrix(cmat, n_true, n_pred):
    """sklearn's `confusion_matrix(y_true, y_pred, normalize="true")` from the [C, C] count matrix (true, pred): restricted to the labels
    that occur in truth or prediction, rows divided by their sums, rows without a truth zero.  Returns (matrix, labels)."""
    cmat = np.asarray(cmat, dtype=np.int64)
    labels = np.nonzero((np.asarray(n_true) > 0) | (np.asarray(n_pred) > 0))[0]
    cm = cmat[np.ix_(labels, labels)]
    with np.errstate(all="ignore"):
        cm = cm / cm.sum(axis=1, keepdims=True)
    return np.nan_to_num(cm), labels


def finish_accuracy(n_hit, n) -> float:
    return float(int(np.sum(n_hit))) / n if n else 0.0


def finish_mean_per_class(n_true, n_hit) -> float:
    """From the MASKED counters (arg-max over the columns whose target is not all zero): mean recall over the classes that occur."""
    n_true, n_hit = np.asarray(n_true, dtype=np.int64), np.asarray(n_hit, dtype=np.int64)
    occurs = np.nonzero(n_true)[0]
    if occurs.size == 0:
        return 0.0
    recalls = [np.float64(n_hit[c]) / n_true[c] for c in occurs]
    return float(np.mean(recalls))


def finish_map(keep, interp) -> float:
    """keep [C] bool: columns whose target is not all zero; interp [C, 11]: the interpolated precisions of every column."""
    keep = np.nonzero(np.asarray(keep))[0]
    if keep.size == 0:
        return 0.0
    per_class = [np.mean(np.array(interp[c], dtype=np.float64)) for c in keep]
    return float(np.mean(per_class))


def finish_roc_auc(n_pos, n_neg, twice_u) -> float:
    vals = []
    for p, n, u in zip(np.asarray(n_pos).tolist(), np.asarray(n_neg).tolist(), np.asarray(twice_u).tolist()):
        if p == 0 or n == 0:
            raise ValueError(ONE_CLASS)
        vals.append(float(np.float64(u / 2.0) / (p * n)))
    return float(np.mean(vals))


def rank_statistics_numpy(scores, positive, thresholds=None):
    """numpy emulation of the column rank kernel for ONE column: (n_pos, n_neg, twice_u, interp[11]) from fp32 scores and a boolean
    positive vector — integer keys, integer run sums, two double divisions per run start.  The tests' yardstick for the kernel, and
    the proof (tests/test_eval_host.py) that the integer formulation reproduces metrics.py bit for bit."""
    thresholds = np.linspace(1, 0, 11, endpoint=True).tolist() if thresholds is None else thresholds
    s = np.ascontiguousarray(scores, dtype=np.float32)
    pos = np.asarray(positive, dtype=bool)
    n = len(s)
    u = s.view(np.uint32).copy()
    u[(u << np.uint32(1)) == 0] = 0                                      # -0.0 -> +0.0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    order = np.argsort(key, kind="stable")
    key, pos = key[order], pos[order]
    n_pos = int(pos.sum())
    interp = np.array([1.0 if th <= 0.0 else 0.0 for th in thresholds])
    if n == 0:
        return 0, 0, 0, interp
    starts = np.r_[0, np.nonzero(key[1:] != key[:-1])[0] + 1].astype(np.int64)
    ends = np.r_[starts[1:], n].astype(np.int64)
    before = np.r_[0, np.cumsum(pos)].astype(np.int64)                   # positives in front of index i
    total = int(np.sum((before[ends] - before[starts]) * (starts + 1 + ends)))
    tp, cnt = n_pos - before[starts], n - starts
    precision = tp.astype(np.float64) / cnt.astype(np.float64)
    recall = tp.astype(np.float64) / np.float64(n_pos) if n_pos else np.ones(len(tp))
    for i, th in enumerate(thresholds):
        reached = precision[th <= recall]
        if reached.size:
            interp[i] = max(interp[i], reached.max())
    return n_pos, n - n_pos, total - n_pos * (n_pos + 1), interp


# ------------------------------------------------------------------------------------------------ Dassl's Classification evaluator
class DeviceClassification:
    """`Classification` of Dassl on device counters (see the module docstring: recalled from upstream).  `task_ranges` ([(lo, hi)] per
    task id) and `task_names` switch on the per-task ranged accuracy when `process` is given task ids."""

    def __init__(self, cfg, lab2cname=None, task_ranges=None, task_names=None):
        self.cfg = cfg
        self._lab2cname = lab2cname
        self._per_class = bool(cfg.TEST.PER_CLASS_RESULT)
        self._cmat = bool(cfg.TEST.COMPUTE_CMAT)
        self._ranges = [tuple(int(v) for v in r) for r in task_ranges] if task_ranges else None
        self._task_names = list(task_names) if task_names else None
        self.reset()

    def reset(self):
        self._buf = self._views = self._lo = self._hi = None
        self._total = 0
        self._task_order = []

    def _allocate(self, n_cls, device):
        import torch
        self._n_cls = n_cls
        self._buf = torch.zeros(5 * n_cls + (n_cls * n_cls if self._cmat else 0), device=device, dtype=torch.int64)
        names = ("n_true", "n_pred", "n_hit", "n_pred_r", "n_hit_r")
        self._views = {k: self._buf[i * n_cls:(i + 1) * n_cls] for i, k in enumerate(names)}
        self._views["cmat"] = self._buf[5 * n_cls:] if self._cmat else None
        if self._ranges:
            self._lo = torch.tensor([r[0] for r in self._ranges], dtype=torch.int32).to(device)
            self._hi = torch.tensor([r[1] for r in self._ranges], dtype=torch.int32).to(device)

    def process(self, logits, labels, tasks=None):
        """logits [B, n_cls] on the device; labels int64 [B] or float rows [B, n_cls] (the row's arg-max); tasks: task id per row."""
        import torch

        from .engine import op_eval_count
        if self._buf is None:
            self._allocate(logits.shape[1], logits.device)
        v = self._views
        ranged = tasks is not None and self._ranges is not None
        task = None
        if ranged:
            tasks = torch.as_tensor(tasks)
            for t in set(tasks.tolist()):                                # the order in which trainers/mvlpt.py:1035 meets the tasks
                if t not in self._task_order:
                    self._task_order.append(t)
            task = tasks.to(device=logits.device, dtype=torch.int32)
        op_eval_count(logits, labels, v["n_true"], v["n_pred"], v["n_hit"], task=task, lo=self._lo if ranged else None,
                      hi=self._hi if ranged else None, n_pred_r=v["n_pred_r"] if ranged else None,
                      n_hit_r=v["n_hit_r"] if ranged else None, cmat=v["cmat"])
        self._total += int(logits.shape[0])

    def evaluate(self):
        results = OrderedDict()
        n = getattr(self, "_n_cls", 0)
        host = self._buf.cpu().numpy() if self._buf is not None else np.zeros(5 * n, dtype=np.int64)      # the one read-back
        c = {k: host[i * n:(i + 1) * n] for i, k in enumerate(("n_true", "n_pred", "n_hit", "n_pred_r", "n_hit_r"))}
        results.update(classification_results(c["n_true"], c["n_pred"], c["n_hit"], self._total))
        correct = int(c["n_hit"].sum())
        print("=> result\n"
              f"* total: {self._total:,}\n"
              f"* correct: {correct:,}\n"
              f"* accuracy: {results['accuracy']:.1f}%\n"
              f"* error: {results['error_rate']:.1f}%\n"
              f"* macro_f1: {results['macro_f1']:.1f}%")
        if self._per_class:
            rows, mean_acc = perclass_table(c["n_true"], c["n_hit"], self._lab2cname)
            print("=> per-class result")
            for label, name, total, hit, acc in rows:
                print(f"* class: {label} ({name})\ttotal: {total:,}\tcorrect: {hit:,}\tacc: {acc:.1f}%")
            print(f"* average: {mean_acc:.1f}%")
            results["perclass_accuracy"] = mean_acc
            results["perclass_table"] = rows
        if self._cmat and n:
            import torch
            cm, labels = confusion_matrix(host[5 * n:].reshape(n, n), c["n_true"], c["n_pred"])
            path = osp.join(self.cfg.OUTPUT_DIR, "cmat.pt")
            import os
            os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
            torch.save(cm, path)
            print(f"Confusion matrix is saved to {path}")
            results["cmat"], results["cmat_labels"] = cm, labels
        if self._ranges is not None:
            per_task = OrderedDict()
            for t in self._task_order:                                   # tasks that were met, in the order they were met
                lo, hi = self._ranges[t]
                name = self._task_names[t] if self._task_names else t
                per_task[name] = 100.0 * float(int(c["n_hit_r"][lo:hi].sum())) / max(int(c["n_true"][lo:hi].sum()), 1)
            results["task_accuracy"] = per_task
        results["counts"] = {k: v.copy() for k, v in c.items()}
        return results


# ------------------------------------------------------------------------------------------------ the ELEVATER metrics
def _host_metric(name, y_true, y_score, rows):
    if rows is not None:
        y_true, y_score = y_true[rows.long()], y_score[rows.long()]
    return M.get_metric(name)(y_true.cpu().numpy(), y_score.float().cpu().numpy())


def _counts(y_true, y_score, rows, masked):
    """(n_true, n_hit) of the arg-max counters over the selected rows; `masked`: over the columns whose target occurs only."""
    import torch

    from .engine import op_eval_count
    n_cls = y_score.shape[1]
    buf = torch.zeros(3 * n_cls, device=y_score.device, dtype=torch.int64)
    n_true, n_pred, n_hit = buf[:n_cls], buf[n_cls:2 * n_cls], buf[2 * n_cls:]
    mask = None
    if masked:                                                           # the column-occurrence pass, then the masked count
        mask = torch.zeros(n_cls, device=y_score.device, dtype=torch.uint8)
        op_eval_count(y_score, y_true, n_true, n_pred, n_hit, rows=rows, col_seen=mask)
        buf.zero_()
    op_eval_count(y_score, y_true, n_true, n_pred, n_hit, rows=rows, col_mask=mask)
    host = buf.cpu().numpy()
    return host[:n_cls], host[2 * n_cls:]


def device_metric(name: str):
    """`metrics.get_metric` for device tensors: fn(y_true, y_score, rows=None) with y_score [N, C] fp32 on the device (a column slice
    is read in place), y_true int64 [N] or float [N, C], rows an optional int32 device list of the rows that count.  The value is the
    double `metrics.py` returns for the same inputs.  A score that is NaN or infinite, or a target that is neither 0 nor 1, sends
    that call to the host functions unchanged."""
    if name not in ("accuracy", "mean-per-class", "11point_mAP", "roc_auc"):
        raise KeyError(f"undefined metric {name!r}")

    def fn(y_true, y_score, rows=None):
        from . import _lib
        from .engine import op_eval_rank_columns
        n = y_score.shape[0] if rows is None else int(rows.numel())
        if y_score.dim() != 2 or (name == "roc_auc" and y_true.dim() == 1):
            return _host_metric(name, y_true, y_score, rows)             # 1-D binary roc_auc stays on the host
        if name == "accuracy":                                           # float rows: their arg-max is the label (trainers/mvlpt.py:1057-1058)
            if n == 0:
                return 0.0
            _, n_hit = _counts(y_true, y_score, rows, masked=False)
            return finish_accuracy(n_hit, n)
        if y_score.numel() == 0 or n == 0:
            return _host_metric(name, y_true, y_score, rows)             # empty inputs: whatever metrics.py makes of them
        if name == "mean-per-class":
            n_true, n_hit = _counts(y_true, y_score, rows, masked=True)
            return finish_mean_per_class(n_true, n_hit)
        out = op_eval_rank_columns(y_score, y_true, rows=rows)
        host = out["packed"].cpu()
        from .engine import unpack_eval_rank
        r = {k: v.numpy() for k, v in unpack_eval_rank(host, y_score.shape[1]).items()}
        if np.any(r["flags"] & (_lib.EVAL_FLAG_NONFINITE | _lib.EVAL_FLAG_SOFT_TARGET)):
            return _host_metric(name, y_true, y_score, rows)
        if name == "roc_auc":
            return finish_roc_auc(r["n_pos"], r["n_neg"], r["twice_u"])
        return finish_map(r["n_pos"] > 0, r["interp"])

    fn.__name__ = f"device_{name}"
    return fn
