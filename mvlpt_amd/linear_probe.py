"""Linear-probe CLIP baseline (lpclip/ of the reference): dump image features, then an L2-regularised multinomial logistic regression
with a search over C, the fits on the device.

`SoftmaxRegression` stands where the reference uses sklearn's LogisticRegression(solver="lbfgs", penalty="l2", C=C).  It minimises

    F(W, b) = (1/N) sum_i [logsumexp(z_i) - z_i[y_i]] + (l2/2) |W|_F^2,   z_i = W x_i + b,   l2 = 1 / (C N),   b unpenalised,

from zero until max|grad F| <= tol.  That is the objective and the stopping rule of sklearn 1.7; the sklearn of the reference's day
minimises C N F, which has the same minimiser and a differently scaled threshold.  Parity is on the minimiser and the stopping rule,
not on the iterates, and NOT on predictions: where the regularisation is weak two correct solvers differ on a few per cent of the
predictions, and at C <= 1e-6 all logits lie within 1e-7 of each other (DESIGN.md row j).
"""
from __future__ import annotations

import os
from typing import Callable, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

HISTORY = 10          # L-BFGS pairs kept
ARMIJO_C1 = 1e-4
WOLFE_DELTA = 0.1
F_NOISE = 1e-6        # relative size of an increase of F that counts as rounding (Hager and Zhang's epsilon)
MAX_TRIALS = 30       # step halvings of one line search
PREDICT_ROWS = 1 << 16


# ------------------------------------------------------------------------------------------------ L-BFGS on flat device vectors
def lbfgs_minimize(evaluate: Callable, theta: torch.Tensor, tol: float, max_iter: int, callback: Optional[Callable] = None):
    """Minimise a convex function from `theta` (flat fp32, any torch device) with L-BFGS (history 10) and Armijo back-tracking
    (c1 = 1e-4, first step min(1, 1/|g|_2), halving, at most 30 trials; under the rounding of F the slope at the trial point
    decides, and a step that leaves fp32 theta where it is never counts).  evaluate(theta, dir) -> (grad tensor, [F, max|g|, g.dir,
    |g|^2] as host floats) is the only source of host numbers per function evaluation; an iteration reads one more scalar, g.d of
    the new direction.  A pair (s, y) with s.y <= 1e-10 y.y is neutralised on the device (rho = 0) instead of being skipped on the host.
    callback(it, event, t, trials, stats), if given, hears of every line search: event is "armijo" | "wolfe" | "failed".
    Returns (theta, n_iter, status, stats of the last accepted point); status is "gtol" | "max_iter" | "line_search"."""
    n = theta.numel()
    dev = theta.device
    S = torch.zeros(HISTORY, n, device=dev, dtype=torch.float32)
    Y = torch.zeros(HISTORY, n, device=dev, dtype=torch.float32)
    rho = torch.zeros(HISTORY, device=dev, dtype=torch.float32)
    gamma = torch.ones((), device=dev, dtype=torch.float32)
    order = []                                       # history slots, oldest first
    g, st = evaluate(theta, None)
    g = g.clone()
    F = st[0]
    if st[1] <= tol:
        return theta, 0, "gtol", st
    d = -g
    gd = -st[3]
    first = True
    status, n_iter = "max_iter", 0
    for it in range(1, max_iter + 1):
        t = min(1.0, 1.0 / max(st[3], 1e-300) ** 0.5) if first else 1.0
        accepted = None
        for trial in range(MAX_TRIALS):
            cand = torch.add(theta, d, alpha=t)
            g_new, st_new = evaluate(cand, d)
            moved = st_new[0] != F or st_new[3] != st[3]      # a step under the spacing of fp32 theta changes nothing: never accept it
            if moved and st_new[0] <= F + ARMIJO_C1 * t * gd:
                accepted = "armijo"
                break
            # The logits are fp32 products, so F carries their rounding (about 1e-7 of its value) while close to the minimiser a step
            # lowers it by g^2 / L, far less.  There the decision passes to the slope, which the evaluation returns (g_new . d): the
            # Armijo test restated for a quadratic model, phi'(t) <= (2 delta - 1) phi'(0) with delta = 0.1 (Hager and Zhang's
            # approximate Wolfe condition).  Their curvature condition is left out on purpose: the search only ever shortens the step,
            # and a direction that is too short (an unpenalised intercept next to heavily penalised weights) must be taken as it is.
            if moved and st_new[0] <= F + F_NOISE * abs(F) and st_new[2] <= (2.0 * WOLFE_DELTA - 1.0) * gd:
                accepted = "wolfe"
                break
            t *= 0.5
        if callback is not None:
            callback(it, accepted or "failed", t, trial + 1, st_new)
        if not accepted:
            if first:
                status = "line_search"
                break
            order, first = [], True                  # drop the history and try the steepest descent once
            gamma.fill_(1.0)
            d = -g
            gd = -st[3]
            continue
        slot = order.pop(0) if len(order) == HISTORY else next(i for i in range(HISTORY) if i not in order)
        torch.mul(d, t, out=S[slot])
        torch.sub(g_new, g, out=Y[slot])
        sy, yy = torch.dot(S[slot], Y[slot]), torch.dot(Y[slot], Y[slot])
        ok = sy > 1e-10 * yy
        rho[slot] = torch.where(ok, 1.0 / torch.where(ok, sy, torch.ones_like(sy)), torch.zeros_like(sy))
        gamma = torch.where(ok, sy / torch.where(ok, yy, torch.ones_like(yy)), gamma)
        order.append(slot)
        theta, F, st, first = cand, st_new[0], st_new, False
        g = g_new.clone()
        n_iter = it
        if st[1] <= tol:
            status = "gtol"
            break
        q = g.clone()
        alpha = {}
        for i in reversed(order):
            alpha[i] = rho[i] * torch.dot(S[i], q)
            q.sub_(alpha[i] * Y[i])
        q.mul_(gamma)
        for i in order:
            beta = rho[i] * torch.dot(Y[i], q)
            q.add_((alpha[i] - beta) * S[i])
        d = -q
        gd = float(torch.dot(g, d))
        if not gd < 0.0:                             # not a descent direction (rounding): steepest descent
            order, first = [], True
            gamma = torch.ones((), device=dev, dtype=torch.float32)
            d = -g
            gd = -st[3]
    return theta, n_iter, status, st


class SoftmaxRegression:
    """L2-regularised multinomial logistic regression fitted on the device, with sklearn's names: fit, predict, coef_ [K, D],
    intercept_ [K] (centred: F does not change under b + c 1), classes_, n_iter_; and converged_, status_ ("gtol" | "max_iter" |
    "line_search").  Fewer than 3 classes raise ValueError: sklearn's two-class model is a different, one-row problem."""

    def __init__(self, C: float = 1.0, max_iter: int = 1000, tol: float = 1e-4, device=None, callback: Optional[Callable] = None):
        self.C, self.max_iter, self.tol = float(C), int(max_iter), float(tol)
        self.device, self.callback = device, callback

    @staticmethod
    def _features(X) -> np.ndarray:
        X = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        if X.ndim != 2 or X.shape[0] < 1:
            raise ValueError("X must be [n_samples, n_features]")
        if X.shape[1] < 4 or X.shape[1] % 4:
            raise ValueError(f"the feature width must be a multiple of 4 (the kernels read 16-byte pieces), got {X.shape[1]}")
        return np.ascontiguousarray(X, dtype=np.float32)

    def fit(self, X, y):
        from . import engine as E
        if not self.C > 0:
            raise ValueError("C must be positive")
        Xh = self._features(X)
        y = np.asarray(y).ravel()
        if y.shape[0] != Xh.shape[0]:
            raise ValueError("X and y disagree on the number of samples")
        self.classes_, yi = np.unique(y, return_inverse=True)
        K = len(self.classes_)
        if K < 3:
            raise ValueError(f"need at least 3 classes, got {K}")
        if yi.min() < 0 or yi.max() >= K:
            raise ValueError("label index out of range")
        N, D = Xh.shape
        dev = torch.device(self.device if self.device is not None else "cuda")
        l2 = 1.0 / (self.C * N)
        with torch.cuda.device(dev):
            Xd = torch.from_numpy(Xh).to(dev)
            yd = torch.from_numpy(yi.astype(np.int32)).to(dev)
            ws = E.softmax_reg_workspace(N, D, K, dev)
            grad = torch.empty(K * D + K, device=dev, dtype=torch.float32)
            stats = torch.empty(4, device=dev, dtype=torch.float64)

            def evaluate(theta, direction):
                E.op_softmax_reg_eval(Xd, yd, theta, l2, dir=direction, grad=grad, stats=stats, ws=ws)
                return grad, stats.tolist()          # the 32-byte read-back

            theta0 = torch.zeros(K * D + K, device=dev, dtype=torch.float32)
            theta, self.n_iter_, self.status_, st = lbfgs_minimize(evaluate, theta0, self.tol, self.max_iter, self.callback)
            self.theta_ = theta.clone()
            self.theta_[K * D:] -= self.theta_[K * D:].mean()
        self.converged_ = self.status_ == "gtol"
        self.objective_, self.max_grad_ = float(st[0]), float(st[1])
        host = self.theta_.cpu().numpy()
        self.coef_, self.intercept_ = host[:K * D].reshape(K, D).copy(), host[K * D:].copy()
        return self

    def predict(self, X, return_margin: bool = False):
        from . import engine as E
        Xh = self._features(X)
        K, D = self.coef_.shape
        if Xh.shape[1] != D:
            raise ValueError(f"X has {Xh.shape[1]} features, the model {D}")
        dev = self.theta_.device
        pred = np.empty(Xh.shape[0], np.int64)
        margin = np.empty(Xh.shape[0], np.float32)
        with torch.cuda.device(dev):
            ws = E.softmax_reg_workspace(min(Xh.shape[0], PREDICT_ROWS), D, K, dev)
            for r0 in range(0, Xh.shape[0], PREDICT_ROWS):
                xd = torch.from_numpy(Xh[r0:r0 + PREDICT_ROWS]).to(dev)
                out = E.op_softmax_reg_predict(xd, self.theta_, margin=return_margin, ws=ws)
                p, m = out if return_margin else (out, None)
                pred[r0:r0 + xd.shape[0]] = p.cpu().numpy()
                if return_margin:
                    margin[r0:r0 + xd.shape[0]] = m.cpu().numpy()
        labels = self.classes_[pred]
        return (labels, margin) if return_margin else labels


def device_fit(X, y, C):
    return SoftmaxRegression(C=C, max_iter=1000).fit(X, y)


# ------------------------------------------------------------------------------------------------ sampling and the search over C
VAL_SHOTS = {1: 1, 2: 2, 4: 4, 8: 4, 16: 4}      # lpclip/linear_probe.py:25
SEARCH_LIST = [1e6, 1e4, 1e2, 1, 1e-2, 1e-4, 1e-6]


def sample_few_shot(labels, num_shot: int, seed_state: np.random.RandomState, classes=None) -> list:
    """Row indices of `num_shot` rows per class, classes ascending, drawn as lpclip/linear_probe.py:33-38 draws them:
    seed_state.choice(rows of the class, size=num_shot, replace=False).  np.random.RandomState(seed) is the stream np.random.seed(seed)
    starts, so a state shared between the train draw and the val draw reproduces the reference's tables bit for bit.  `classes`
    defaults to np.unique(labels); the reference samples val over the TRAIN classes."""
    labels = np.asarray(labels)
    picked = []
    for label in (np.unique(labels) if classes is None else classes):
        rows = np.where(labels == label)[0]
        if len(rows) < num_shot:
            raise ValueError(f"class {label} has {len(rows)} rows, fewer than {num_shot} shots")
        picked.extend(seed_state.choice(rows, size=num_shot, replace=False))
    return picked


def linear_probe(train, val, test, num_step: int = 8, num_run: int = 10, shots: Sequence[int] = (1, 2, 4, 8, 16),
                 fit_fn: Optional[Callable] = None, dataset: str = "", feature_dir: str = "clip_feat", report_dir: str = "report",
                 log: Callable = print) -> dict:
    """The few-shot sweep of lpclip/linear_probe.py:25-129, oddities included: per shot count and seed 1 .. num_run, sample train and
    then val rows from one np.random stream, fit at the seven C of SEARCH_LIST, take the FIRST best validation accuracy as the peak,
    then num_step rounds on [0.1 peak, 10 peak]: a fit at each end every round (nothing is reused), the left end wins a tie, the
    interval is halved in log10 and comes back through np.power.  The test accuracy of each round's winner goes to
    `{report_dir}/{feature_dir}_s{num_step}r{num_run}_details.txt`, mean and std of the last round per shot count to
    `..._s{num_step}r{num_run}.txt`, both appended in the reference's line formats.

    train / val / test: (features [n, D], labels [n]).  fit_fn(X, y, C) -> object with .predict(X); the default fits on the device.
    Returns {"trace": [(shot, seed, step, c_left, c_right, c_final, test_acc)], "summary": {shot: (mean, std)}, "fits": count}."""
    fit_fn = device_fit if fit_fn is None else fit_fn
    (train_feature, train_label), (val_feature, val_label), (test_feature, test_label) = [
        (np.asarray(f), np.asarray(l)) for f, l in (train, val, test)]
    os.makedirs(report_dir, exist_ok=True)
    stem = os.path.join(report_dir, "{}_s{}r{}".format(feature_dir, num_step, num_run))
    trace, summary, fits = [], {}, 0

    def val_accuracy(C):
        clf = fit_fn(fewshot_train_feature, fewshot_train_label, C)
        pred = clf.predict(fewshot_val_feature)
        return clf, sum(pred == fewshot_val_label) / len(fewshot_val_label)

    for num_shot in shots:
        test_acc_step_list = np.zeros([num_run, num_step])
        for seed in range(1, num_run + 1):
            state = np.random.RandomState(seed)
            log(f"-- Seed: {seed} --------------------------------------------------------------")
            all_label_list = np.unique(train_label)
            selected = sample_few_shot(train_label, num_shot, state, all_label_list)
            fewshot_train_feature, fewshot_train_label = train_feature[selected], train_label[selected]
            val_selected = sample_few_shot(val_label, VAL_SHOTS[num_shot], state, all_label_list)
            fewshot_val_feature, fewshot_val_label = val_feature[val_selected], val_label[val_selected]

            acc_list = []
            for c_weight in SEARCH_LIST:
                acc_list.append(val_accuracy(c_weight)[1])
                fits += 1
            log(acc_list)
            c_peak = SEARCH_LIST[np.argmax(acc_list)]
            c_left, c_right = 1e-1 * c_peak, 1e1 * c_peak

            for step in range(num_step):
                log(f"{dataset}, {num_shot} Shot, Round {step}: {c_left}/{c_right}")
                clf_left, acc_left = val_accuracy(c_left)
                log("Val accuracy (Left): {:.2f}".format(100 * acc_left))
                clf_right, acc_right = val_accuracy(c_right)
                log("Val accuracy (Right): {:.2f}".format(100 * acc_right))
                fits += 2
                entered = (c_left, c_right)
                if acc_left < acc_right:
                    c_final, clf_final = c_right, clf_right
                    c_left = 0.5 * (np.log10(c_right) + np.log10(c_left))
                    c_right = np.log10(c_right)
                else:
                    c_final, clf_final = c_left, clf_left
                    c_right = 0.5 * (np.log10(c_right) + np.log10(c_left))
                    c_left = np.log10(c_left)
                pred = clf_final.predict(test_feature)
                test_acc = 100 * sum(pred == test_label) / len(pred)
                log("Test Accuracy: {:.2f}".format(test_acc))
                test_acc_step_list[seed - 1, step] = test_acc
                with open(stem + "_details.txt", "a+") as writer:
                    writer.write("{}, seed {}, {} shot, weight {}, test_acc {:.2f}\n".format(dataset, seed, num_shot, c_final, test_acc))
                trace.append((num_shot, seed, step, entered[0], entered[1], c_final, test_acc))
                c_left, c_right = np.power(10, c_left), np.power(10, c_right)
        last = test_acc_step_list[:, -1]
        summary[num_shot] = (float(np.mean(last)), float(np.std(last)))
        save_line = "{}, {} Shot, Test acc stat: {:.2f} ({:.2f})\n".format(dataset, num_shot, np.mean(last), np.std(last))
        log(save_line)
        with open(stem + ".txt", "a+") as writer:
            writer.write(save_line)
    return {"trace": trace, "summary": summary, "fits": fits}


# ------------------------------------------------------------------------------------------------ features and their files
def extract_features(clip, batches: Iterable) -> Tuple[np.ndarray, np.ndarray]:
    """(features [n, embed] fp32, labels [n] int64) of an iterable of (images, labels): FrozenCLIP.encode_image per batch, un-normalised
    as the reference's clip_model.visual(data) is (lpclip/feat_extractor.py:155), rows in input order.  The tower is whatever the
    FrozenCLIP holds: the reference hard-codes RN50 (mvlpt_amd.weights.RESNET_ARCHS["RN50"], the convolutional tower of
    mvlpt_create_resnet); any ViT of ARCHS works the same way, under the activation the FrozenCLIP was built with
    (FrozenCLIP(activation=read_activation(cfg)): MODEL.BACKBONE.ACTIVATION)."""
    feats, labels = [], []
    for images, lab in batches:
        feats.append(clip.encode_image(images).float().cpu().numpy())
        labels.extend(int(v) for v in np.asarray(torch.as_tensor(lab).cpu()).ravel())
        if feats[-1].shape[0] != len(labels) - sum(f.shape[0] for f in feats[:-1]):
            raise ValueError("a batch has a different number of images and labels")
    if not feats:
        raise ValueError("no batches")
    return np.concatenate(feats, 0), np.asarray(labels, np.int64)


def save_split(directory: str, split: str, features, labels) -> str:
    """`{directory}/{split}.npz` with the reference's keys feature_list / label_list (lpclip/feat_extractor.py:163-167)."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"{split}.npz")
    np.savez(path[:-4], feature_list=np.asarray(features), label_list=np.asarray(labels))
    return path


def load_split(directory: str, split: str) -> Tuple[np.ndarray, np.ndarray]:
    with np.load(os.path.join(directory, f"{split}.npz")) as f:
        return f["feature_list"], f["label_list"]
