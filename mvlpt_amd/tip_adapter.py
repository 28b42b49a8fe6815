"""Tip-Adapter and Tip-Adapter-F (Zhang et al., ECCV 2022) on the HIP engine: `TipAdapterHead` and `--trainer TipAdapter`.

Training-free few-shot CLIP: zero-shot logits plus a key-value cache of the few-shot image features,

    logits = s f W^T + alpha * exp(-beta (1 - f K^T)) @ one_hot(key labels),      f, K rows and W rows of unit length.

The published code forms the [N, NK] affinities and multiplies them with the one-hot matrix; here the keys are kept SORTED BY CLASS with
a CSR table `key_ptr`, and one fused kernel (mvlpt_op_tip_logits, csrc/tip.hip) does the product, the exponential and the per-class sum.
`search_hp` is the published 200 x 20 grid over (beta, alpha) as ONE call (mvlpt_op_tip_search): the affinities are formed once and
alpha enters in the arg-max alone.  Tip-Adapter-F (`fit`) fine-tunes the keys with AdamW under a cosine schedule over all steps, the
image tower frozen (mvlpt_op_tip_train_fwd / _bwd); the keys are not re-normalised while training, as published.

The cache wants every few-shot image once, in the same order on every pass, under the train augmentation: the trainer reads it from the
loader's ordered pass (mvlpt_amd.data.DeviceLoader.ordered), not from the shuffled, drop_last epochs that `fit` trains on.

`TipAdapterHead` needs no trainer: it stands next to `linear_probe.extract_features` the way `SoftmaxRegression` does
(tools/tip_adapter.py runs it on saved `{split}.npz` features).
"""
from __future__ import annotations

import math
import os
import os.path as osp
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from .config import CfgNode
from .trainer import build_optimizer
from .zsclip import ZeroshotCLIP

MAX_NB, MAX_NA = 256, 32        # MVLPT_TIP_MAX_NB, MVLPT_TIP_MAX_NA: the largest grid of one search
ADAMW_WEIGHT_DECAY = 0.01       # torch.optim.AdamW's default: the published code passes lr and eps alone


def search_grid(scale: Sequence[float] = (7.0, 3.0), step: Sequence[int] = (200, 20)) -> Tuple[list, list]:
    """The published grid: beta_i = i (scale[0] - 0.1) / step[0] + 0.1 for i < step[0], alpha_j likewise from scale[1], step[1]."""
    if len(scale) != 2 or len(step) != 2 or int(step[0]) < 1 or int(step[1]) < 1:
        raise ValueError("search grid: scale = (beta scale, alpha scale) and step = (beta steps, alpha steps), steps at least 1")
    betas = [i * (float(scale[0]) - 0.1) / int(step[0]) + 0.1 for i in range(int(step[0]))]
    alphas = [i * (float(scale[1]) - 0.1) / int(step[1]) + 0.1 for i in range(int(step[1]))]
    return betas, alphas


def first_maximum(counts) -> Tuple[int, int]:
    """(b, a) of the first maximum in beta-major order: the published loop updates its best only on `>`."""
    counts = np.asarray(counts)
    flat = int(np.argmax(counts.reshape(-1)))
    return flat // counts.shape[1], flat % counts.shape[1]


def key_table(labels, n_cls: int) -> Tuple[np.ndarray, np.ndarray]:
    """(stable order of the keys by class, key_ptr int32 [n_cls + 1]); labels outside [0, n_cls) raise ValueError."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    if labels.size == 0:
        raise ValueError("the cache needs at least one key")
    if labels.min() < 0 or labels.max() >= n_cls:
        raise ValueError(f"key labels must lie in [0, {n_cls}), got {labels.min()} .. {labels.max()}")
    order = np.argsort(labels, kind="stable")
    key_ptr = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=n_cls))]).astype(np.int32)
    return order, key_ptr


class _Keys(nn.Module):
    """The cache keys as the module build_optimizer takes."""

    def __init__(self, keys: torch.Tensor):
        super().__init__()
        self.keys = nn.Parameter(keys)


class TipAdapterHead:
    """The cache head.  engine: mvlpt_amd.engine.Engine; text_features [C, D]: the unit rows of the zero-shot classifier
    (ZeroshotCLIP.text_features); logit_scale_exp: exp(logit_scale).  Features given to any method are UN-normalised image features
    [n, D] (FrozenCLIP.encode_image, or the rows extract_features saved); the head normalises them with the engine's x / |x| op."""

    def __init__(self, engine, text_features: torch.Tensor, logit_scale_exp: float, alpha: float = 1.0, beta: float = 5.5,
                 fused: bool = False):
        self.engine = engine
        self.text_features = text_features.float().contiguous()
        self.device = self.text_features.device
        self.n_cls, self.dim = self.text_features.shape
        self.logit_scale_exp, self.alpha, self.beta, self.fused = float(logit_scale_exp), float(alpha), float(beta), bool(fused)
        self.keys = self.key_labels = self.key_ptr = None
        self.history = []

    # ------------------------------------------------------------------------------------------------ the cache
    def _unit(self, x) -> torch.Tensor:
        x = torch.as_tensor(x).to(self.device).float()
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"features must be [n, {self.dim}], got {tuple(x.shape)}")
        return self.engine.text_ensemble(x.contiguous().view(1, *x.shape))      # one template: x / |x|

    def _set_cache(self, keys: torch.Tensor, labels) -> "TipAdapterHead":
        labels = np.asarray(torch.as_tensor(labels).cpu()).astype(np.int64).ravel()
        if labels.shape[0] != keys.shape[0]:
            raise ValueError(f"{keys.shape[0]} keys but {labels.shape[0]} labels")
        order, key_ptr = key_table(labels, self.n_cls)
        self.keys = keys.to(self.device).float()[torch.from_numpy(order).to(self.device)].contiguous()
        self.key_labels = torch.from_numpy(labels[order])
        self.key_ptr = torch.from_numpy(key_ptr).to(self.device)
        return self

    def from_features(self, features, labels, n_cls: Optional[int] = None) -> "TipAdapterHead":
        """The cache of one pass: keys = unit(unit(features)), stably sorted by class."""
        if n_cls is not None and int(n_cls) != self.n_cls:
            raise ValueError(f"n_cls = {n_cls} but the text classifier has {self.n_cls} classes")
        return self._set_cache(self._unit(self._unit(features)), labels)

    def build_cache(self, clip, batches_fn: Callable, augment_epochs: int = 10) -> "TipAdapterHead":
        """The published build_cache_model: `augment_epochs` passes over batches_fn() (which yields (images, labels) in the same order
        on every call; the augmentation differs), each feature normalised, the mean over the passes normalised again."""
        if int(augment_epochs) < 1:
            raise ValueError("augment_epochs must be at least 1")
        total, labels0 = None, None
        for epoch in range(int(augment_epochs)):
            feats, labels = [], []
            for images, lab in batches_fn():
                feats.append(self._unit(clip.encode_image(images)))
                labels.extend(int(v) for v in np.asarray(torch.as_tensor(lab).cpu()).ravel())
            if not feats:
                raise ValueError("batches_fn() yielded no batch")
            feats = torch.cat(feats, 0)
            if feats.shape[0] != len(labels):
                raise ValueError("a batch has a different number of images and labels")
            if labels0 is None:
                labels0, total = labels, feats
            else:
                if labels != labels0:
                    raise ValueError(f"augmentation epoch {epoch}: the labels differ from epoch 0 (batches_fn must keep its order)")
                total = total + feats
        return self._set_cache(self._unit(total / float(int(augment_epochs))), labels0)

    def _need_cache(self):
        if self.keys is None:
            raise RuntimeError("the Tip-Adapter cache is empty: build_cache, from_features or load_state_dict first")

    # ------------------------------------------------------------------------------------------------ inference
    def logits(self, features) -> torch.Tensor:
        self._need_cache()
        return self.engine.tip_logits(self._unit(features), self.keys, self.key_ptr, self.text_features, self.logit_scale_exp,
                                      self.alpha, self.beta)

    def predict(self, features) -> torch.Tensor:
        return self.logits(features).argmax(1)

    def search_hp(self, features, labels, scale: Sequence[float] = (7.0, 3.0), step: Sequence[int] = (200, 20)):
        """The published search_hp over the grid of `search_grid`: sets alpha and beta to the FIRST grid point with the most correct
        rows and returns (beta, alpha, accuracy in per cent, counts int64 [step[0], step[1]])."""
        self._need_cache()
        betas, alphas = search_grid(scale, step)
        if len(betas) > MAX_NB or len(alphas) > MAX_NA:
            raise ValueError(f"search grid {len(betas)} x {len(alphas)}: one search takes at most {MAX_NB} betas and {MAX_NA} alphas")
        F = self._unit(features)
        y = torch.as_tensor(labels).to(self.device).to(torch.int32).view(-1)
        if y.shape[0] != F.shape[0]:
            raise ValueError(f"{F.shape[0]} feature rows but {y.shape[0]} labels")
        if int(y.min()) < 0 or int(y.max()) >= self.n_cls:
            raise ValueError(f"labels must lie in [0, {self.n_cls})")
        bt = torch.tensor(betas, dtype=torch.float32, device=self.device)
        at = torch.tensor(alphas, dtype=torch.float32, device=self.device)
        counts = self.engine.tip_search(F, y, self.keys, self.key_ptr, self.text_features, self.logit_scale_exp, bt, at)
        counts = counts.cpu().numpy().astype(np.int64)
        b, a = first_maximum(counts)
        self.beta, self.alpha = betas[b], alphas[a]
        return self.beta, self.alpha, 100.0 * float(counts[b, a]) / F.shape[0], counts

    # ------------------------------------------------------------------------------------------------ Tip-Adapter-F
    def _optimizer(self, lr: float, eps: float):
        holder = _Keys(self.keys.clone())
        cfg = CfgNode(NAME="adamw", LR=float(lr), WEIGHT_DECAY=ADAMW_WEIGHT_DECAY, FUSED=self.fused)
        flat = None
        if self.fused:
            from .distributed import FlatGradients, FlatParameters
            flat = (FlatParameters(holder.parameters()), FlatGradients(holder.parameters()))
            holder.keys.grad = flat[1].views[0]
        optim = build_optimizer(holder, cfg, flat)
        for g in optim.param_groups:
            g["eps"] = float(eps)
        return holder, optim

    def train_step(self, features, labels, keys: Optional[torch.Tensor] = None):
        """(loss [1], correct int32 [1], dK [NK, D]) of the cross-entropy of the Tip logits with respect to `keys` (default: the cache)."""
        self._need_cache()
        keys = self.keys if keys is None else keys
        y = torch.as_tensor(labels).to(self.device).to(torch.int32).view(-1)
        loss, correct = self.engine.tip_train_fwd(self._unit(features), y, keys, self.key_ptr, self.text_features,
                                                  self.logit_scale_exp, self.alpha, self.beta)
        return loss, correct, self.engine.tip_train_bwd()

    def accuracy(self, features, labels, keys: Optional[torch.Tensor] = None) -> float:
        self._need_cache()
        F = self._unit(features)
        z = self.engine.tip_logits(F, self.keys if keys is None else keys, self.key_ptr, self.text_features, self.logit_scale_exp,
                                   self.alpha, self.beta)
        y = torch.as_tensor(labels).to(self.device).view(-1)
        return 100.0 * float((z.argmax(1) == y).sum()) / F.shape[0]

    @torch.no_grad()
    def fit(self, clip, batches_fn: Callable, epochs: int = 20, lr: float = 1e-3, eps: float = 1e-4, eval_set=None) -> "TipAdapterHead":
        """Tip-Adapter-F: the keys are an fp32 parameter initialised from the cache; AdamW(lr, eps) with CosineAnnealingLR over
        epochs * steps, stepped every iteration.  Each step encodes its batch with the frozen tower, without gradients.
        eval_set = (features, labels): the keys of the epoch with the best accuracy on it are kept (a later epoch must be strictly
        better); None keeps the last epoch's.  self.history: (epoch, mean loss, train accuracy, eval accuracy or None) per epoch."""
        self._need_cache()
        epochs = int(epochs)
        if epochs < 1:
            raise ValueError("epochs must be at least 1")
        first = batches_fn()
        steps = len(first) if hasattr(first, "__len__") else sum(1 for _ in first)      # an unsized loader costs one pass to count
        if steps < 1:
            raise ValueError("batches_fn() yielded no batch")
        holder, optim = self._optimizer(lr, eps)
        total, it = epochs * steps, 0
        best_acc, best_keys = -math.inf, None
        self.history = []
        for epoch in range(epochs):
            loss_sum = torch.zeros(1, device=self.device)
            hit_sum = torch.zeros(1, dtype=torch.int64, device=self.device)
            n_rows = 0
            for images, lab in batches_fn():
                for g in optim.param_groups:                                            # CosineAnnealingLR(T_max = total), eta_min 0
                    g["lr"] = 0.5 * float(lr) * (1.0 + math.cos(math.pi * it / total))
                loss, correct, dK = self.train_step(clip.encode_image(images), lab, holder.keys.data)
                if holder.keys.grad is None:
                    holder.keys.grad = dK
                else:
                    holder.keys.grad.copy_(dK)
                optim.step()
                loss_sum += loss
                hit_sum += correct
                n_rows += int(torch.as_tensor(lab).numel())
                it += 1
            acc = None
            if eval_set is not None:
                acc = self.accuracy(eval_set[0], eval_set[1], holder.keys.data)
                if acc > best_acc:
                    best_acc, best_keys = acc, holder.keys.data.clone()
            self.history.append((epoch, float(loss_sum) / steps, 100.0 * int(hit_sum) / max(n_rows, 1), acc))
        self.keys = (best_keys if best_keys is not None else holder.keys.data.clone()).contiguous()
        return self

    # ------------------------------------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        self._need_cache()
        return {"keys": self.keys.detach().cpu().clone(), "key_labels": self.key_labels.clone(), "alpha": float(self.alpha),
                "beta": float(self.beta)}

    def load_state_dict(self, sd: dict) -> "TipAdapterHead":
        keys = torch.as_tensor(sd["keys"]).float()
        if keys.dim() != 2 or keys.shape[1] != self.dim:
            raise ValueError(f"keys must be [NK, {self.dim}], got {tuple(keys.shape)}")
        self._set_cache(keys, sd["key_labels"])      # sorted already: the stable sort keeps the order
        self.alpha, self.beta = float(sd["alpha"]), float(sd["beta"])
        return self


# ---------------------------------------------------------------------------------------------------- the trainer
def tip_settings(cfg) -> dict:
    """cfg.TRAINER.TIP, checked; every refusal is a ValueError that names its key."""
    T = cfg.TRAINER.TIP
    if cfg.TRAINER.MVLPT.VPT.N_CTX != 0:
        raise ValueError("TRAINER.MVLPT.VPT.N_CTX != 0: Tip-Adapter caches the features of the frozen, prompt-free image tower; visual "
                         "prompts are not offered, set VPT.N_CTX 0")
    if cfg.DATASET.MULTITASK:
        raise ValueError("DATASET.MULTITASK: Tip-Adapter's cache and its search run over ONE class list; multitask class ranges are "
                         "not offered, run one dataset at a time")
    out = {"augment_epoch": int(T.AUGMENT_EPOCH), "alpha": float(T.INIT_ALPHA), "beta": float(T.INIT_BETA),
           "search": bool(T.SEARCH_HP), "scale": [float(v) for v in T.SEARCH_SCALE], "step": [int(v) for v in T.SEARCH_STEP],
           "finetune": bool(T.FINETUNE), "epochs": int(T.TRAIN_EPOCH), "lr": float(T.LR), "eps": float(T.EPS)}
    if out["augment_epoch"] < 1:
        raise ValueError(f"TRAINER.TIP.AUGMENT_EPOCH = {T.AUGMENT_EPOCH!r}: at least one pass over the few-shot set")
    if len(out["scale"]) != 2 or len(out["step"]) != 2 or min(out["step"]) < 1:
        raise ValueError("TRAINER.TIP.SEARCH_SCALE / SEARCH_STEP: two values each (beta, alpha), steps at least 1")
    if out["finetune"] and out["epochs"] < 1:
        raise ValueError(f"TRAINER.TIP.TRAIN_EPOCH = {T.TRAIN_EPOCH!r}: at least one epoch of fine-tuning")
    if not out["lr"] > 0 or not out["eps"] > 0:
        raise ValueError("TRAINER.TIP.LR and TRAINER.TIP.EPS must be positive")
    return out


class _Batches:
    """(images, labels) of a trainer's loader, on the trainer's device; sized, so that `fit` knows its steps without a pass.
    ordered: every item once in dataset order with nothing dropped, what the cache is built from.  A loader that shuffles per epoch
    offers such a pass as `ordered()` (mvlpt_amd.data.DeviceLoader: its train transform, fresh draws); one without the method (a list
    of resident batches) already serves the same batches on every pass."""

    def __init__(self, trainer, loader, ordered: bool = False):
        self.trainer, self.loader = trainer, loader
        self.ordered = ordered and hasattr(loader, "ordered")

    def __len__(self):
        return len(self.loader.ordered_batches()) if self.ordered else len(self.loader)

    def __iter__(self):
        for batch in (self.loader.ordered() if self.ordered else self.loader):
            image, label, _ = self.trainer.parse_batch_train(batch)
            yield image, label


class TipAdapter(ZeroshotCLIP):
    """`--trainer TipAdapter`: zero-shot CLIP (one template, TRAINER.ZSCLIP.TEMPLATES) plus the cache head.  `train()` builds the cache
    from the few-shot train loader (TRAINER.TIP.AUGMENT_EPOCH passes), optionally fine-tunes the keys (FINETUNE: Tip-Adapter-F), then
    searches (beta, alpha) on the validation loader.  test() and the device evaluators are MVLPT's: model_inference returns the Tip
    logits."""

    MODEL_NAME = "tip_adapter"

    def check_cfg(self, cfg):
        super().check_cfg(cfg)
        tip_settings(cfg)

    def build_model(self):
        super().build_model()
        s = tip_settings(self.cfg)
        self.head = TipAdapterHead(self.clip_model.engine, self.text_features, self.logit_scale_exp, alpha=s["alpha"], beta=s["beta"],
                                   fused=bool(self.cfg.OPTIM.get("FUSED", False)))

    def _batches(self, loader, ordered: bool = False):
        return _Batches(self, loader, ordered)

    def _features(self, loader):
        feats, labels = [], []
        for image, label in self._batches(loader):
            feats.append(self.clip_model.encode_image(image).float())
            labels.append(label.view(-1))
        return torch.cat(feats, 0), torch.cat(labels, 0)

    @torch.no_grad()
    def train(self):
        s = tip_settings(self.cfg)
        self.head.build_cache(self.clip_model, lambda: self._batches(self.train_loader_x, ordered=True), s["augment_epoch"])
        print(f"Tip-Adapter cache: {self.head.keys.shape[0]} keys over {self.head.n_cls} classes, {s['augment_epoch']} passes")
        held_out = self.val_loader
        if held_out is None:
            held_out = self.test_loader
            if held_out is not None and (s["search"] or s["finetune"]):
                print("Tip-Adapter: no validation loader, the search runs on the TEST loader (as the published code does for ImageNet)")
        eval_set = self._features(held_out) if held_out is not None and (s["search"] or s["finetune"]) else None
        if s["finetune"]:
            self.head.fit(self.clip_model, lambda: self._batches(self.train_loader_x), s["epochs"], s["lr"], s["eps"], eval_set=eval_set)
            for epoch, loss, acc, held in self.head.history:
                print(f"epoch [{epoch + 1}/{s['epochs']}] loss {loss:.4f} acc {acc:.2f}" + ("" if held is None else f" held-out {held:.2f}"))
        if s["search"] and eval_set is not None:
            beta, alpha, acc, _ = self.head.search_hp(eval_set[0], eval_set[1], s["scale"], s["step"])
            print(f"Tip-Adapter search: beta {beta:.4f} alpha {alpha:.4f} accuracy {acc:.2f}")
        self.epoch = s["epochs"] - 1 if s["finetune"] else 0
        self.save_model(self.epoch, self.output_dir)
        self.end_of_epoch_loop()
        return None if self.cfg.TEST.NO_TEST or self.test_loader is None else self.test()

    @torch.no_grad()
    def model_inference(self, image, task=None):
        return self.head.logits(self.clip_model.encode_image(image))

    def forward_backward(self, batch):
        raise RuntimeError("Tip-Adapter has no per-batch step of the generic loop: call train()")

    def save_model(self, epoch, directory, is_best=False, val_result=None, model_name=""):
        if self.rank != 0 or not directory:
            return
        d = osp.join(directory, self.MODEL_NAME)
        os.makedirs(d, exist_ok=True)
        ckpt = {"state_dict": self.head.state_dict(), "epoch": epoch + 1, "val_result": val_result}
        torch.save(ckpt, osp.join(d, model_name or f"model.pth.tar-{epoch + 1}"))
        torch.save(ckpt, osp.join(d, "model-best.pth.tar"))      # what load_model(directory, epoch=None) opens

    def load_model(self, directory, epoch=None):
        if not directory:
            print("Note that load_model() is skipped as no pretrained model is given")
            return
        path = osp.join(directory, self.MODEL_NAME, "model-best.pth.tar" if epoch is None else "model.pth.tar-" + str(epoch))
        if not osp.exists(path):
            raise FileNotFoundError('Model not found at "{}"'.format(path))
        self.head.load_state_dict(torch.load(path, map_location="cpu")["state_dict"])
