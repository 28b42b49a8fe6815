"""The MVLPT trainer's CoCoOp route (trainers/mvlpt.py with TRAINER.MVLPT.COCOOP.N_CTX != 0) on the HIP engine.

`MVLPT.build_model` picks :class:`CustomCLIP` of this module iff ``cfg.TRAINER.MVLPT.COCOOP.N_CTX != 0``; every other configuration goes
through `mvlpt_amd.model` exactly as before (whose classes keep refusing COCOOP.N_CTX != 0).  Class names, constructor arguments and
``prompt_learner.state_dict()`` keys are the reference's (``cocoop_ctx``, ``meta_net.linear{1,2}.{weight,bias}``, ``token_prefix``,
``token_suffix``, + ``vpt_embeddings[_deep]`` / ``vpt_proj.*`` with visual prompts), so checkpoints interoperate.

What the route does (trainers/mvlpt.py:541-581): image tower (with visual prompts when VPT.N_CTX != 0) -> normalise -> ``meta_net`` ->
``ctx_shifted = cocoop_ctx + bias`` (one context block per image) -> one text feature set PER IMAGE -> cosine logits -> per-task mask.
The reference runs one text tower per image in a Python loop and multiplies every logit outside the image's task by 0.  Here

* under ``DATASET.MULTITASK_LABEL_PERTASK`` image b runs ONLY the sequences of its own task's class range [lo_b, hi_b)
  (the ranged mvlpt_text_fwd / mvlpt_logits_ranged_fwd): a masked logit is exactly 0 and carries no gradient, so its sequence is never
  computed.  ``CustomCLIP.ranged_text = False`` runs every range full (B x n_cls sequences, CoCoOp's tower) and a multiplicative mask
  instead — the same logits, for comparison and as an escape hatch.  Without the per-task mask every range is [0, n_cls).
* the batch is cut into chunks of consecutive images whose text tower fits ``max_text_workspace_bytes`` (sized over the chunk's OWN
  sequence count, not B * n_cls).  ``forward`` returns logits, so the backward arrives later: with ONE chunk the forward saves its
  activations and the backward uses them; with MORE than one chunk the forward runs without saving and the backward RE-RUNS every
  chunk's text forward with saving right before that chunk's backward — one extra text forward per step, the price of keeping only
  one chunk's activations alive.
* ``meta_net``, the normalisation in front of it and ``ctx + bias`` stay on torch autograd (as in mvlpt_amd.cocoop); the text side is
  one autograd node (image features, shifted contexts) -> logits whose backward hands out d ctx_shifted AND d image features (the
  ranged head's dimg); the image tower with visual prompts is a second node whose incoming gradient is the sum autograd forms from the
  head's dimg and the ``meta_net`` path.

Deviations: parameters are fp32 masters for every COCOOP.PREC (the reference halves ``meta_net`` under fp16); COOP.N_CTX != 0
together with COCOOP.N_CTX != 0 (a ``ctx`` the reference builds and never uses on this branch) is refused; step pipelining and class
sharding do not apply to per-image text features.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .model import (FrozenCLIP, PretokenizedPrompts, VisualPromptSide, _CrossEntropyFn, class_prompt_tables, class_range_tables,
                    deep_text_prompts, image_conditioned_ctx, register_class_tables)
from .model import MultitaskVLPromptLearner as _BasePromptLearner
from .per_image_text import PerImageTextCLIP, class_ranges
from .schedule import check_forward_is_current


class MultitaskVLPromptLearner(_BasePromptLearner):
    """trainers/mvlpt.py:138-325 for COCOOP.N_CTX != 0 (:260-289, :313-314).  The visual-prompt parameters and `forward_mvlpt_proj`
    are the base class's; the text side is `cocoop_ctx` + `meta_net` with an "end" layout over `cocoop_n_ctx`."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, pretokenized: Optional[PretokenizedPrompts] = None):
        nn.Module.__init__(self)
        n_cls = len(classnames)
        T = cfg.TRAINER.MVLPT
        cocoop_n_ctx, vpt_n_ctx = T.COCOOP.N_CTX, T.VPT.N_CTX
        if cocoop_n_ctx == 0:
            raise ValueError("mvlpt_amd.mvlpt_cocoop is the COCOOP.N_CTX != 0 route; use mvlpt_amd.model otherwise")
        deep_text_prompts(cfg, clip_model.arch)      # COOP.N_DEEP > 0 is refused on this route
        if T.COOP.N_CTX != 0:
            raise NotImplementedError("COOP.N_CTX != 0 together with COCOOP.N_CTX != 0: the reference builds a `ctx` its logits never "
                                      "depend on (trainers/mvlpt.py:556-571); set COOP.N_CTX 0")
        arch = clip_model.arch
        self._init_visual_prompts(cfg, clip_model)                                      # :165-201, as the base class
        self.ctx = None
        self.mvlpt_proj = nn.Identity()                                                 # :235 (no COOP ctx: nothing to project)

        ctx_vectors, self.meta_net, prompt_prefix, cocoop_n_ctx = image_conditioned_ctx(    # :262-286; fp32 masters (module docstring)
            clip_model, cocoop_n_ctx, T.COCOOP.CTX_INIT, arch.transformer_width, arch.embed_dim, clip_model.dtype)
        self.cocoop_ctx = nn.Parameter(ctx_vectors)

        self.vpt_n_ctx, self.coop_n_ctx, self.cocoop_n_ctx = vpt_n_ctx, 0, cocoop_n_ctx
        self.class_token_position = T.COOP.CLASS_TOKEN_POSITION
        tables = class_prompt_tables(clip_model, classnames, pretokenized, prompt_prefix, cfg.TRAINER.CUT_CONTEXTLEN)   # :292-307
        # construct_prompts (:327-346) is cat([prefix, ctx, suffix]): the "end" layout of the HIP text tower
        register_class_tables(self, n_cls, tables, cocoop_n_ctx, "end")                 # token_suffix: CLS, EOS (:313-314)

    def forward(self, im_features):
        """forward_cocoop (:348-374) up to the shifted contexts [B, n_ctx, ctx_dim]; the prompts are assembled by the HIP tower."""
        bias = self.meta_net(im_features).unsqueeze(1)       # (batch, 1, ctx_dim)
        return self.cocoop_ctx.unsqueeze(0) + bias           # (batch, n_ctx, ctx_dim)


class _ImageTowerFn(torch.autograd.Function):
    """The image tower with visual prompts as an autograd node: mvlpt_image_fwd(save_for_bwd) / mvlpt_image_bwd."""

    @staticmethod
    def forward(fctx, model: "CustomCLIP", image, vpt_emb, vpt_deep_emb, grad_on=True):
        need = grad_on and bool(fctx.needs_input_grad[2] or fctx.needs_input_grad[3])
        img = model.engine.image_fwd(image, vpt_emb, vpt_deep_emb, save_for_bwd=need)
        fctx.model, fctx.generation, fctx.vpt_shape = model, model._fwd_generation, vpt_emb.shape
        return img

    @staticmethod
    def backward(fctx, dimg):
        check_forward_is_current(fctx.model, fctx.generation)
        dvpt, ddeep = fctx.model.engine.image_bwd(dimg.contiguous())
        return None, None, dvpt.view(fctx.vpt_shape), ddeep, None


class _TextSideFn(torch.autograd.Function):
    """(image features [B, e], shifted contexts [B, n_ctx, dt]) -> logits [B, n_cls]: per chunk the ranged text tower (every range
    full on the dense route) and the ranged head.  See the module docstring for the one-chunk / recompute arrangement of the backward."""

    @staticmethod
    def forward(fctx, model: "CustomCLIP", img, ctx_shifted, lo, hi, mask, grad_on=True):
        need_img = grad_on and bool(fctx.needs_input_grad[1])
        need_ctx = grad_on and bool(fctx.needs_input_grad[2])
        model.last_sequences = sum(hi) - sum(lo)
        if not (need_img or need_ctx):
            logits = model.ranged_logits(img, ctx_shifted, lo, hi)
            model.last_recompute = False
        else:
            chunks = model.chunks(lo, hi, model.text_len(ctx_shifted), save_for_bwd=True)
            save = len(chunks) == 1                          # more than one chunk: the backward runs each chunk's forward again
            logits = torch.empty(len(lo), model.prompt_learner.n_cls, device=img.device, dtype=torch.float32)
            for g0, g1, S in chunks:
                if S == 0:
                    logits[g0:g1] = 0.0
                else:
                    logits[g0:g1] = model.chunk_logits(img, ctx_shifted, lo, hi, g0, g1, save)
            model.last_chunks, model.last_recompute = len(chunks), not save
            fctx.model, fctx.lo, fctx.hi, fctx.chunks, fctx.mask = model, lo, hi, chunks, mask
            fctx.need_img, fctx.need_ctx, fctx.saved_in_engine = need_img, need_ctx, save
            fctx.generation = model._fwd_generation
            fctx.save_for_backward(img, ctx_shifted)
        return logits if mask is None else logits * mask     # the dense route's select_index (trainers/mvlpt.py:581)

    @staticmethod
    def backward(fctx, dlogits):
        model = fctx.model
        eng = model.engine
        if fctx.saved_in_engine:
            check_forward_is_current(model, fctx.generation)
        img, ctx_shifted = fctx.saved_tensors
        dl = dlogits.contiguous() if fctx.mask is None else (dlogits * fctx.mask).contiguous()
        dimg = torch.zeros_like(img) if fctx.need_img else None
        dctx = torch.zeros_like(ctx_shifted) if fctx.need_ctx else None
        for g0, g1, S in fctx.chunks:
            if S == 0:
                continue                                     # empty ranges only: no logit depends on anything
            if not fctx.saved_in_engine:                     # more than one chunk: this chunk's forward again, saved this time
                model.chunk_logits(img, ctx_shifted, fctx.lo, fctx.hi, g0, g1, fctx.need_ctx)
            di, dtxt = eng.logits_ranged_bwd(dl[g0:g1], need_img=fctx.need_img, need_txt=fctx.need_ctx)
            if fctx.need_img:
                dimg[g0:g1] = di
            if fctx.need_ctx:
                dctx[g0:g1] = eng.text_bwd(dtxt)
        return None, dimg, dctx, None, None, None, None


class CustomCLIP(VisualPromptSide, PerImageTextCLIP):
    """trainers/mvlpt.py:517-583 for COCOOP.N_CTX != 0: `forward(image, task=None)` returns the logits [B, n_cls]."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, dm=None, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        self.prompt_learner = MultitaskVLPromptLearner(cfg, classnames, clip_model, pretokenized)
        self._init_engine_side(cfg, clip_model)      # precision raised to split_all, as in mvlpt_amd.cocoop.CustomCLIP
        self.ranged_text = True              # False: every range full (B x n_cls sequences) + multiplicative mask
        self.last_sequences = 0
        self.last_recompute = False
        self._fwd_generation = 0
        self.multi_task_label_pertask = cfg.DATASET.MULTITASK_LABEL_PERTASK
        self.class_index_pertask_start = self.class_index_pertask_end = None
        if self.multi_task_label_pertask:
            self.class_index_pertask_start, self.class_index_pertask_end = class_range_tables(dm)      # kept on the CPU

    # ---- what does not apply to per-image text features
    def enable_class_sharding(self, rank: int, world: int) -> None:
        if world > 1:
            raise NotImplementedError("class sharding does not apply to the COCOOP.N_CTX != 0 route: every image has its own text "
                                      "features, there is no shared [n_cls, e] matrix to shard")

    def prefetch_image_features(self, image, stop_block=None, cu_cap=None) -> bool:
        """Step pipelining is off on this route (the image features feed meta_net, and with visual prompts they are not constants)."""
        return False

    def split_active(self) -> bool:
        return False

    def drop_prefetch(self) -> None:
        pass

    def _image_side(self, image):
        """(image features [B, e], shifted contexts [B, n_ctx, ctx_dim]): the image tower with its visual prompts, then :561-563."""
        _, vpt_emb, vpt_emb_deep = self.projected_prompts(batch=image.shape[0])  # :541 (no COOP ctx: the parameters themselves)
        if vpt_emb is not None:
            img = _ImageTowerFn.apply(self, image, vpt_emb, vpt_emb_deep, torch.is_grad_enabled())
        else:
            img = self.engine.image_fwd(image, None, None, save_for_bwd=False)   # frozen, prompt-free image tower
        imf = img / img.norm(dim=-1, keepdim=True)                               # :561 (meta_net's input)
        return img, self.prompt_learner(imf)                                     # :563, :361-364

    @torch.no_grad()
    def image_contexts(self, image) -> torch.Tensor:
        """cocoop_ctx + meta_net(image features) [B, n_ctx, ctx_dim], as an evaluation forward computes them: the prompt learner is put
        in eval mode for the call (no VPT dropout, nothing drawn from the RNG) and restored.  It counts as a forward: the image tower
        runs and replaces the activations the engine keeps, so the backward of an earlier forward raises the stale-forward error."""
        pl = self.prompt_learner
        was_training = pl.training
        pl.eval()
        self._fwd_generation += 1
        try:
            return self._image_side(image.to(self.clip_model.device))[1]
        finally:
            pl.train(was_training)

    def forward(self, image, task=None):
        pl = self.prompt_learner
        B = image.shape[0]
        self._fwd_generation += 1
        img, ctx_shifted = self._image_side(image)
        lo, hi = class_ranges(task, self.class_index_pertask_start, self.class_index_pertask_end, B, pl.n_cls)
        mask = None
        if not self.ranged_text and self.multi_task_label_pertask:
            idx = torch.arange(pl.n_cls).unsqueeze(0)
            mask = ((idx >= torch.tensor(lo).unsqueeze(1)) & (idx < torch.tensor(hi).unsqueeze(1))).float().to(image.device)
            lo, hi = self.full_ranges(B)
        return _TextSideFn.apply(self, img, ctx_shifted, lo, hi, mask, torch.is_grad_enabled())

    def cross_entropy(self, logits, label):
        """HIP replacement for ``F.cross_entropy(output, label)`` (trainers/mvlpt.py:931)."""
        return _CrossEntropyFn.apply(self, logits, label)
