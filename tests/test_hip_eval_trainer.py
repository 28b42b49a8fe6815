"""`MVLPT.test()` on device counters (-m gpu): the same trainer on the same three batches with TEST.DEVICE_METRICS True and False.
The return value, `last_results` and `last_task_results` are compared with `==` (the device route produces the integer counts the
host route's numpy calls are functions of), and `last_eval` — Dassl's figures, which the host route does not have — against numpy
counts of the model's own logits."""
import os

import numpy as np
import pytest
import torch

from mvlpt_amd import evaluator as E

pytestmark = pytest.mark.gpu


def make_trainer(tmp_path, classes, tasks=None, elevater=False, metric_names=None, evalkey="average", B=16, **test_keys):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    from mvlpt_amd.weights import ARCHS, make_state_dict
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = B
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.TRAINER.MVLPT.COOP.N_CTX = 4
    if tasks:
        cfg.DATASET.MULTITASK = True
        cfg.DATASET.MULTITASK_LABEL_PERTASK = True
        cfg.DATASET.MULTITASK_EVALKEY = evalkey
    cfg.DATASET.COOP = not elevater
    for k, v in test_keys.items():
        cfg.TEST[k] = v
    dm = SyntheticDataManager(cfg, classes, 3, task_class_counts=tasks, device="cuda", seed=3, elevater=elevater, metric_names=metric_names)
    tr = MVLPT(cfg, dm=dm, clip_state_dict=make_state_dict(ARCHS["tiny"], seed=9))
    tr.test_loader = tr.train_loader_x                                   # 3 batches
    return tr


def both_routes(tr):
    out = []
    for device in (True, False):
        tr.cfg.TEST.DEVICE_METRICS = device
        out.append((tr.test(), dict(tr.last_results), dict(tr.last_task_results), tr.last_eval))
    (v1, r1, t1, ev), (v0, r0, t0, ev0) = out
    assert ev is not None and ev0 is None                                # the device route ran, and only when asked to
    assert v1 == v0 and r1 == r0 and t1 == t0, (v1, v0, r1, r0, t1, t0)
    return v1, r1, t1, ev


def logits_and_labels(tr):
    xs, ys = [], []
    with torch.no_grad():
        for batch in tr.test_loader:
            img, lab, task = tr.parse_batch_test(batch)
            xs.append(tr.model_inference(img, task=task).float().cpu().numpy())
            ys.append((lab.argmax(1) if lab.dim() > 1 else lab).cpu().numpy())
    return np.concatenate(xs), np.concatenate(ys)


def check_dassl_figures(ev, x, y):
    n = x.shape[1]
    pred = np.argmax(x, axis=1)
    n_true, n_pred, n_hit = np.bincount(y, minlength=n), np.bincount(pred, minlength=n), np.bincount(y[y == pred], minlength=n)
    for k, want in (("n_true", n_true), ("n_pred", n_pred), ("n_hit", n_hit)):
        assert np.array_equal(ev["counts"][k], want), k
    want = E.classification_results(n_true, n_pred, n_hit, len(y))
    assert (ev["accuracy"], ev["error_rate"], ev["macro_f1"]) == (want["accuracy"], want["error_rate"], want["macro_f1"])
    assert ev["accuracy"] == 100.0 * int((pred == y).sum()) / len(y)
    return n_true, n_pred, n_hit, pred


def test_coop_single_task_with_per_class_table_and_confusion_matrix(tmp_path, capsys):
    tr = make_trainer(tmp_path, classes=6, PER_CLASS_RESULT=True, COMPUTE_CMAT=True)
    value, results, per_task, ev = both_routes(tr)
    assert list(results) == ["accuracy"] and per_task == {}
    x, y = logits_and_labels(tr)
    n_true, n_pred, n_hit, pred = check_dassl_figures(ev, x, y)
    rows, mean_acc = E.perclass_table(n_true, n_hit)
    assert ev["perclass_accuracy"] == mean_acc and [r[2:] for r in ev["perclass_table"]] == [r[2:] for r in rows]
    cm = torch.load(os.path.join(str(tmp_path), "cmat.pt"), weights_only=False)
    counts = np.zeros((6, 6), np.int64)
    np.add.at(counts, (y, pred), 1)
    want, labels = E.confusion_matrix(counts, n_true, n_pred)
    assert np.array_equal(cm, want) and np.array_equal(ev["cmat_labels"], labels)
    text = capsys.readouterr().out                                       # the lines the reference's parse_test_res.py reads
    for line in ("=> result", f"* total: {len(y):,}", f"* accuracy: {value:.1f}%", "* macro_f1: ", "=> per-class result", "* average: "):
        assert line in text, line


def test_coop_multitask_three_tasks(tmp_path):
    tr = make_trainer(tmp_path, classes=9, tasks=[3, 2, 4])
    value, results, per_task, ev = both_routes(tr)
    assert list(results) == ["average"] and set(per_task) == {"task0", "task1", "task2"}
    assert not os.path.exists(os.path.join(str(tmp_path), "cmat.pt"))    # TEST.COMPUTE_CMAT is off by default
    x, y = logits_and_labels(tr)
    check_dassl_figures(ev, x, y)
    for t, (lo, hi) in enumerate([(0, 3), (3, 5), (5, 9)]):
        sel = (y >= lo) & (y < hi)
        assert per_task[f"task{t}"] == 100.0 * float(int((lo + np.argmax(x[sel][:, lo:hi], axis=1) == y[sel]).sum())) / int(sel.sum())


def test_coop_multitask_evalkey_names_a_task(tmp_path):
    tr = make_trainer(tmp_path, classes=9, tasks=[3, 2, 4], evalkey="task1")
    value, results, per_task, _ = both_routes(tr)
    assert list(results) == ["task1"] and value == per_task["task1"]


@pytest.mark.parametrize("name", ["accuracy", "mean-per-class", "11point_mAP", "roc_auc"])
def test_elevater_single_task(tmp_path, name):
    tr = make_trainer(tmp_path, classes=5, elevater=True, metric_names=name)
    value, results, per_task, _ = both_routes(tr)
    assert list(results) == [name] and per_task == {}


@pytest.mark.parametrize("evalkey", ["average", "task2"])
def test_elevater_multitask_with_a_metric_per_task(tmp_path, evalkey):
    tr = make_trainer(tmp_path, classes=9, tasks=[3, 2, 4], elevater=True, evalkey=evalkey, B=32,
                      metric_names=["accuracy", "11point_mAP", "mean-per-class"])
    value, results, per_task, _ = both_routes(tr)
    assert list(results) == [evalkey] and set(per_task) == {"task0", "task1", "task2"}
    tr.dm._metric_name["task1"] = "roc_auc"                              # the fourth metric on a task's slice and row list
    from mvlpt_amd.metrics import roc_auc
    tr.dm._metric["task1"] = roc_auc
    both_routes(tr)


def test_cocoop_and_zero_shot_trainers_inherit_the_route(tmp_path):
    from mvlpt_amd import zsclip
    from mvlpt_amd.cocoop import CoCoOp
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import SyntheticDataManager
    from mvlpt_amd.weights import ARCHS, make_state_dict
    weights = make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True)
    for cls, name, sd in ((CoCoOp, "CoCoOp", None), (zsclip.ZeroshotCLIP, "ZeroshotCLIP", weights)):
        cfg = get_cfg_default()
        cfg.MODEL.BACKBONE.NAME = "tiny"
        cfg.INPUT.SIZE = (32, 32)
        cfg.TRAINER.NAME = name
        cfg.TRAINER.COCOOP.N_CTX = 4
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
        cfg.OUTPUT_DIR = str(tmp_path)
        dm = SyntheticDataManager(cfg, num_classes=6, steps_per_epoch=3, seed=3)
        tr = cls(cfg, dm=dm, clip_state_dict=sd)
        tr.test_loader = dm.train_loader_x
        value, results, _, ev = both_routes(tr)
        x, y = logits_and_labels(tr)
        check_dassl_figures(ev, x, y)
