"""Test-time prompt tuning (TPT, Shu et al., NeurIPS 2022; built on the CoOp code base) on the HIP engine: `--trainer TPT`.

Label-free and evaluation-only.  For every test image: V augmented views (view 0 the clean test view), the k most confident views
are kept, STEPS AdamW steps on the image's OWN copy of the text context minimise the entropy of their averaged prediction, the image
is classified with the tuned context, and the context is reset.  The published implementation tunes one image at a time; here a batch
of G test images is ONE ranged text tower with `ctx [G, n_ctx, dt]` and every class range full (the ranged mvlpt_text_fwd, CoCoOp's
situation), followed by the fused entropy head (mvlpt_op_tpt_head_fwd / _bwd, csrc/tpt.hip).  AdamW on the flat [G, n_ctx, dt] tensor
is element-wise, so G images tuned side by side are G independent TPT problems, and chunks of images (sized by the text-workspace
planner CoCoOp uses) are exact.

The generic context `ctx0 [n_ctx, dt]` lives in the CoOp prompt learner (mvlpt_amd.model.MultitaskVLPromptLearner): the same
state_dict keys, so a CoOp checkpoint loads through MVLPT.load_model and COOP.CTX_INIT works.  `tune` never modifies it.

Deviations (DESIGN.md row o): the views are RandomResizedCrop + flip (the published recipe for the ImageNet variants; AugMix views are
not offered); weight decay is torch.optim.AdamW's default 0.01, as in the published code, which passes only the learning rate.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from .config import CfgNode
from .model import FrozenCLIP, MultitaskVLPromptLearner, PretokenizedPrompts
from .per_image_text import PerImageTextCLIP
from .trainer import MVLPT, TrainerX, build_optimizer

MAX_VIEWS = 128              # MVLPT_TPT_MAX_VIEWS
ADAMW_WEIGHT_DECAY = 0.01    # torch.optim.AdamW's default: the published code passes the learning rate alone


def tpt_settings(cfg, world_size: int = 1) -> Tuple[int, int, int, float]:
    """(n_views, k, steps, lr) of cfg.TRAINER.TPT, checked; every refusal is a ValueError that names its key."""
    T, M = cfg.TRAINER.TPT, cfg.TRAINER.MVLPT
    if M.COOP.CSC:
        raise ValueError("TRAINER.MVLPT.COOP.CSC: test-time prompt tuning tunes ONE generic context per image; class-specific contexts "
                         "are not offered, set COOP.CSC False")
    if M.VPT.N_CTX != 0:
        raise ValueError("TRAINER.MVLPT.VPT.N_CTX != 0: the image tower of test-time prompt tuning is frozen, prompt-free and runs "
                         "once per image; visual prompts are not offered, set VPT.N_CTX 0")
    if M.COCOOP.N_CTX != 0:
        raise ValueError("TRAINER.MVLPT.COCOOP.N_CTX != 0: test-time prompt tuning starts from a generic context; set COCOOP.N_CTX 0")
    if M.COOP.get("N_DEEP", 0) != 0:
        raise ValueError("TRAINER.MVLPT.COOP.N_DEEP != 0: the ranged text tower has no deep prompts; set COOP.N_DEEP 0")
    n_views = T.N_VIEWS
    if isinstance(n_views, bool) or not isinstance(n_views, int) or not 1 <= n_views <= MAX_VIEWS:
        raise ValueError(f"TRAINER.TPT.N_VIEWS = {n_views!r}: the number of views per image lies in 1 .. {MAX_VIEWS}")
    p = float(T.SELECTION_P)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"TRAINER.TPT.SELECTION_P = {T.SELECTION_P!r}: the kept fraction of the views lies in (0, 1]")
    steps = int(T.STEPS)
    if steps < 0:
        raise ValueError(f"TRAINER.TPT.STEPS = {T.STEPS!r}: the number of tuning steps cannot be negative")
    if T.PREC not in ("fp16", "fp32", "amp"):
        raise ValueError(f"TRAINER.TPT.PREC = {T.PREC!r}: fp16 | fp32 | amp")
    if world_size > 1:
        raise ValueError(f"class sharding over {world_size} ranks: every test image tunes against all classes on one device; run "
                         "test-time prompt tuning on one rank")
    return n_views, max(1, int(n_views * p)), steps, float(T.LR)


def prompt_cfg(cfg):
    """The config the CoOp prompt learner is built from: TRAINER.MVLPT.COOP as it stands when it asks for a context (N_CTX != 0: a
    CoOp checkpoint's setting), else TRAINER.TPT's N_CTX / CTX_INIT with the class at the end ("a photo of a <class>.")."""
    c = cfg.clone()
    coop = c.TRAINER.MVLPT.COOP
    if coop.N_CTX == 0:
        coop.N_CTX, coop.CTX_INIT, coop.CLASS_TOKEN_POSITION = int(cfg.TRAINER.TPT.N_CTX), cfg.TRAINER.TPT.CTX_INIT, "end"
    if coop.N_CTX <= 0 and not coop.CTX_INIT:
        raise ValueError("TRAINER.TPT.N_CTX must be positive (or CTX_INIT given): there is no context to tune")
    return c


class _Contexts(nn.Module):
    """The per-image contexts of one `tune` call, as the module build_optimizer takes."""

    def __init__(self, ctx: torch.Tensor):
        super().__init__()
        self.ctx = nn.Parameter(ctx)


class CustomCLIP(PerImageTextCLIP):
    """The model of the TPT trainer: `tune(views)` -> logits [G, n_cls]."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        self.n_views, self.k, self.steps, self.lr = tpt_settings(cfg)
        self.prompt_learner = MultitaskVLPromptLearner(prompt_cfg(cfg), classnames, clip_model, pretokenized)
        self._init_engine_side(cfg, clip_model)
        self.optim_cfg = CfgNode(NAME="adamw", LR=self.lr, WEIGHT_DECAY=ADAMW_WEIGHT_DECAY, FUSED=bool(cfg.OPTIM.get("FUSED", False)))
        self.last_loss = self.last_selected = self.last_entropy = None
        self.last_dctx = None

    def enable_class_sharding(self, rank: int, world: int) -> None:
        if world > 1:
            raise ValueError(f"class sharding over {world} ranks: every test image tunes against all classes on one device; run "
                             "test-time prompt tuning on one rank")

    def image_contexts(self, image):
        raise RuntimeError("test-time prompt tuning has no image-conditioned context to interpret: the tuned contexts are reset "
                           "after every image")

    def _optimizer(self, ctx: torch.Tensor):
        holder = _Contexts(ctx)
        flat = None
        if self.optim_cfg.FUSED:
            from .distributed import FlatGradients, FlatParameters
            flat = (FlatParameters(holder.parameters()), FlatGradients(holder.parameters()))
            holder.ctx.grad = flat[1].views[0]
        return holder, build_optimizer(holder, self.optim_cfg, flat)

    def tune_step(self, feats: torch.Tensor, ctx: torch.Tensor):
        """One forward + backward over every image, chunk by chunk: (loss [G], H [G, V], sel [G, k], dctx [G, n_ctx, dt]) for the
        contexts `ctx` against the (fixed) view features `feats` [G, V, e].  Per-image losses are independent: chunking is exact."""
        eng = self.engine
        G, V = feats.shape[0], feats.shape[1]
        lo, hi = self.full_ranges(G)
        chunks = self.chunks(lo, hi, self.text_len(ctx), save_for_bwd=True)
        loss = torch.empty(G, device=feats.device, dtype=torch.float32)
        H = torch.empty(G, V, device=feats.device, dtype=torch.float32)
        sel = torch.empty(G, self.k, device=feats.device, dtype=torch.int32)
        dctx = torch.empty_like(ctx)
        for g0, g1, _ in chunks:
            txt = self.text_chunk(ctx, lo, hi, g0, g1, save=True)
            loss[g0:g1], H[g0:g1], sel[g0:g1] = eng.tpt_head_fwd(feats[g0:g1], txt, self.logit_scale_exp, self.k)
            dctx[g0:g1] = eng.text_bwd(eng.tpt_head_bwd())
        self.last_chunks = len(chunks)
        return loss, H, sel, dctx

    @torch.no_grad()
    def tune(self, views: torch.Tensor) -> torch.Tensor:
        """views [G, V, 3, R, R], view 0 the clean test view -> logits [G, n_cls] of view 0 under each image's tuned context."""
        if views.dim() != 5:
            raise ValueError(f"tune takes views [G, V, 3, R, R] (view 0 the test view), got {tuple(views.shape)}")
        eng, pl = self.engine, self.prompt_learner
        G, V = views.shape[0], views.shape[1]
        if not self.k <= V:
            raise ValueError(f"{V} views per image but k = {self.k} (TRAINER.TPT.N_VIEWS * SELECTION_P) are to be kept")
        # 1. the features never change: one image tower over the G * V views, whatever STEPS is
        feats = eng.image_fwd(views.reshape(G * V, *views.shape[2:]), None, None, save_for_bwd=False).view(G, V, -1)
        # 2. every image its own copy of the context, fresh optimizer state
        ctx0 = pl.ctx.detach()
        ctx = ctx0.unsqueeze(0).expand(G, *ctx0.shape).clone()
        holder = optim = None
        # 3. STEPS steps; the selection is recomputed every step
        for _ in range(self.steps):
            if optim is None:
                holder, optim = self._optimizer(ctx)
                ctx = holder.ctx.data
            self.last_loss, self.last_entropy, self.last_selected, dctx = self.tune_step(feats, ctx)
            self.last_dctx = dctx
            if holder.ctx.grad is None:
                holder.ctx.grad = dctx
            else:
                holder.ctx.grad.copy_(dctx)
            optim.step()
            ctx = holder.ctx.data
        # 4. classify view 0 with the tuned contexts; the chunk count reported is the tuning steps' when there were any
        tuning_chunks = self.last_chunks
        out = self.ranged_logits(feats[:, 0].contiguous(), ctx, *self.full_ranges(G))
        if self.steps != 0:
            self.last_chunks = tuning_chunks
        self.last_ctx = ctx
        return out

    def forward(self, views, task=None):
        return self.tune(views)


class TPT(MVLPT):
    """Test-time prompt tuning as a trainer: evaluation only (nothing is trained or saved), `test()` is MVLPT's, so the device
    metrics and DeviceClassification come with it.  The test loader serves views (DeviceDataManager.request_views)."""

    def check_cfg(self, cfg):
        tpt_settings(cfg, getattr(self, "world_size", 1))

    def build_data_loader(self):
        super().build_data_loader()
        self.train_loader_x = self.dm.train_loader_x          # nothing is trained: no look-ahead loader
        request = getattr(self.dm, "request_views", None)
        if request is not None:
            request(tpt_settings(self.cfg)[0])

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames if cfg.DATASET.COOP else list(self.dm.lab2cname.values())
        pretok = getattr(self.dm, "pretokenized", None)
        prec = "split_all" if cfg.TRAINER.TPT.PREC == "fp32" else cfg.TRAINER.MVLPT.GRAD_PRECISION
        self.model = CustomCLIP(cfg, classnames, MVLPT.frozen_clip(self, prec, include_token_embedding=True), pretokenized=pretok)
        self.train_prompt_learner_only()        # freezes the rest, INIT_WEIGHTS, device; the optimizer it builds is never stepped

    def forward_backward(self, batch):
        raise RuntimeError("test-time prompt tuning has nothing to train: call test()")

    def parse_batch_test(self, batch):
        image, label, tasks = self.parse_batch_train(batch)
        return image, label, None

    @torch.no_grad()
    def model_inference(self, input, task=None):
        """`input`: the views [B, V, 3, R, R] the test loader serves."""
        return self.model.tune(input)

    def end_of_epoch_loop(self):
        TrainerX.end_of_epoch_loop(self)

    def after_epoch(self):
        TrainerX.after_epoch(self)
