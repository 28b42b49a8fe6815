"""What the models with one text context per image share: mvlpt_amd.cocoop.CustomCLIP, mvlpt_amd.mvlpt_cocoop.CustomCLIP and
mvlpt_amd.tpt.CustomCLIP.  Image g brings its own context `ctx[g]` and a class range [lo_g, hi_g), so a batch is ONE ranged text tower
over sum(hi - lo) sequences (the ranged mvlpt_text_fwd), cut into chunks of consecutive images whose workspace fits
`max_text_workspace_bytes`.  Here live the chunk planner, one chunk's tower (the only caller of Engine.text_fwd_ranged) and the loop
of a forward that keeps nothing for a backward.  A forward that saves differs in what follows the tower (CoCoOp: loss and backward
per chunk; the MVLPT route: logits now, backward later; TPT: the entropy head), so those three loops stay with their models, each
written over `chunks` and `text_chunk`.
"""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.nn as nn

from . import _lib
# DEFAULT_MAX_TEXT_WORKSPACE_BYTES: workspace budget of a per-image text tower (not a reference key).  A chunk holds as many images as
# fit it (mvlpt_text_workspace_bytes); ViT-B/16 with 100 classes needs 1.67 GiB per image for a training step.
from .model import (DEFAULT_MAX_TEXT_WORKSPACE_BYTES, MAX_SEQUENCES_PER_TOWER, FrozenCLIP, _text_inputs, apply_text_act_ckpt,
                    apply_text_grad_len)


def class_ranges(task, start, end, B: int, n_cls: int) -> Tuple[List[int], List[int]]:
    """Host class range [lo_b, hi_b) of every image: its task's range (`start` / `end` indexed by task id, trainers/mvlpt.py:575-576)
    or [0, n_cls) without the per-task mask (`start is None`).  `task` stays on the CPU: nothing is read back from the device."""
    if start is None:
        return [0] * B, [n_cls] * B
    t = task.cpu().long() if torch.is_tensor(task) else torch.as_tensor(task).long()
    if t.shape != (B,):
        raise ValueError(f"task must hold one task id per image ({B}), got shape {tuple(t.shape)}")
    return start[t].tolist(), end[t].tolist()


def chunk_bounds(widths: List[int], fits) -> List[Tuple[int, int, int]]:
    """Cut the images into chunks of consecutive images (g0, g1, S): greedily the longest run whose sequence count S = sum of the
    range widths satisfies `fits(S)`; a single image that does not fit still makes a chunk of its own.  S may be 0 (empty ranges only)."""
    out, g0, S = [], 0, 0
    for g, w in enumerate(widths):
        if g > g0 and S + w > 0 and not fits(S + w):
            out.append((g0, g, S))
            g0, S = g, 0
        S += w
    out.append((g0, len(widths), S))
    return out


class PerImageTextCLIP(nn.Module):
    """The engine side of the constructor, the chunked ranged text tower and `interpret_images`.  A subclass sets `prompt_learner`
    first and provides `image_contexts`.  Contexts are `ctx` [B, n_ctx, ctx_dim]; `lo` / `hi` are host lists over the whole batch."""

    def _init_engine_side(self, cfg, clip_model: FrozenCLIP) -> None:
        self.tokenized_prompts = self.prompt_learner.tokenized_prompts
        self.clip_model = clip_model
        self.engine = clip_model.engine
        self.text_act_ckpt = apply_text_act_ckpt(cfg, self.engine)      # TRAINER.ACT_CKPT: the chunk planner sees the smaller workspace
        self.logit_scale = clip_model.logit_scale
        self.logit_scale_exp = float(clip_model.logit_scale.exp())
        self.dtype = clip_model.dtype
        self.trim_text_to_eot = False        # mvlpt_amd.model.CustomCLIP's switch, same default
        self.text_grad_to_eot = bool(cfg.TRAINER.MVLPT.get("TEXT_GRAD_TO_EOT", True))      # likewise
        self.max_text_workspace_bytes = DEFAULT_MAX_TEXT_WORKSPACE_BYTES
        # Precision: the image features are meta_net's input and every text row carries a gradient, so under the
        # default mode (split operands only in towers kept for a backward) the ViT-B/16 fixture's ctx / meta_net gradients land at
        # 0.9-1.3e-3 of the reference; with split operands in every tower (MVLPT_PREC_SPLIT_ALL) at <= 8.3e-4.  CoCoOp therefore
        # raises the engine's default mode to split_all ("fast", an explicit request for single operands, is left alone).
        # (An image tower with heads wider than 64 has single operands only: its mode stays split_grad, under which the text tower,
        # which carries the gradient, runs on pairs all the same.)
        if self.engine.precision == _lib.PREC_SPLIT_GRAD and getattr(clip_model.arch, "vision_head_width", 64) == 64:
            self.engine.set_precision("split_all")
        self.last_chunks = 0
        self.last_ncorrect = None

    # ---- the planner
    def full_ranges(self, B: int) -> Tuple[List[int], List[int]]:
        """(lo, hi) of B images that each run against every class."""
        return [0] * B, [self.prompt_learner.n_cls] * B

    def chunks(self, lo: List[int], hi: List[int], L: int, save_for_bwd: bool) -> List[Tuple[int, int, int]]:
        """[(g0, g1, S)]: consecutive images whose text tower over S = sum(hi - lo) sequences fits `max_text_workspace_bytes`."""
        eng, budget = self.engine, self.max_text_workspace_bytes
        return chunk_bounds([b - a for a, b in zip(lo, hi)],
                            lambda S: S <= MAX_SEQUENCES_PER_TOWER and eng.text_workspace_bytes(S, L, save_for_bwd) <= budget)

    def images_per_chunk(self, B: int, L: int, save_for_bwd: bool) -> int:
        """Number of images (<= B) in a chunk when every range is full: the first chunk `chunks` cuts from B such images."""
        g0, g1, _ = self.chunks(*self.full_ranges(B), L, save_for_bwd)[0]
        return g1 - g0

    def text_len(self, ctx) -> int:
        """Positions per sequence of the tower `text_chunk` runs for `ctx` (what `chunks` takes as L)."""
        return _text_inputs(self, self.prompt_learner, ctx.shape[1])[1].shape[1]

    # ---- one chunk
    def text_chunk(self, ctx, lo: List[int], hi: List[int], g0: int, g1: int, save: bool):
        """Text features [S, embed] of images [g0, g1): image g's context against classes [lo[g], hi[g]).  `save` keeps the tower's
        activations for Engine.text_bwd, which then stops behind the class table's largest EOT position."""
        pl = self.prompt_learner
        suffix, layout = _text_inputs(self, pl, ctx.shape[1])
        if save:
            apply_text_grad_len(self, pl)
        return self.engine.text_fwd_ranged(pl.token_prefix, suffix, ctx[g0:g1], layout, pl.eot, lo[g0:g1], hi[g0:g1], save_for_bwd=save)

    def chunk_logits(self, img, ctx, lo: List[int], hi: List[int], g0: int, g1: int, save: bool):
        """`text_chunk` and the ranged cosine head over the same ranges: logits [g1 - g0, n_cls], 0 outside an image's range."""
        txt = self.text_chunk(ctx, lo, hi, g0, g1, save)
        return self.engine.logits_ranged_fwd(img[g0:g1], txt, self.logit_scale_exp, lo[g0:g1], hi[g0:g1], self.prompt_learner.n_cls)

    # ---- the loop of a forward nothing is kept from
    @torch.no_grad()
    def ranged_logits(self, img, ctx, lo: List[int], hi: List[int]):
        """Logits [B, n_cls] of image features `img` [B, embed] under the contexts `ctx`, chunk by chunk; sets `last_chunks`."""
        chunks = self.chunks(lo, hi, self.text_len(ctx), save_for_bwd=False)
        out = torch.empty(len(lo), self.prompt_learner.n_cls, device=img.device, dtype=torch.float32)
        for g0, g1, S in chunks:
            if S == 0:
                out[g0:g1] = 0.0                             # empty ranges only: there is no tower to run
            else:
                out[g0:g1] = self.chunk_logits(img, ctx, lo, hi, g0, g1, save=False)
        self.last_chunks = len(chunks)
        return out

    def interpret_images(self, images, topk: int = 5):
        """Nearest vocabulary words of every image's own contexts: [B][n_ctx] lists of (word, distance), B * n_ctx rows in ONE
        nearest-token call (mvlpt_amd.interpret)."""
        from .interpret import nearest_words
        return nearest_words(self.clip_model, self.image_contexts(images), topk)
