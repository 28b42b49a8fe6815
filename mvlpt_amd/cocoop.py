"""CoCoOp (trainers/cocoop.py) on the HIP engine: image-conditioned prompts, `--trainer CoCoOp`.

Same class names, constructor arguments and ``prompt_learner.state_dict()`` keys as the reference (``ctx``,
``meta_net.linear{1,2}.{weight,bias}``, ``token_prefix``, ``token_suffix``), so CoCoOp checkpoints interoperate.

Every image g gets its own context ``ctx + meta_net(img_g / |img_g|)``, so the text tower runs over B x n_cls sequences per
step.  The reference loops over the images in Python (trainers/cocoop.py:184-189) and trains at batch size 1; here the
whole batch (or the largest chunk of it whose workspace fits ``CustomCLIP.max_text_workspace_bytes``) is ONE ranged tower with
every image's class range full, [0, n_cls) (the ranged mvlpt_text_fwd: the [n_cls, ...] prefix / suffix / layout tables are read per
image, never copied), followed by the ranged cosine head over the same ranges (mvlpt_logits_ranged_fwd / _bwd) and the existing
cross-entropy kernel: the entries the MVLPT trainer's COCOOP.N_CTX != 0 route (mvlpt_amd.mvlpt_cocoop) calls with per-task ranges.
``meta_net`` and ``ctx + bias`` (a few thousand FLOPs per image, trainable) stay on torch autograd, as the UPT projection does.

Deviations: parameters are fp32 masters for every PREC (the reference halves ``meta_net`` under fp16); the
prompt learner's ``forward`` returns the shifted contexts [B, n_ctx, ctx_dim] — the prompt assembly is a HIP kernel.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .model import FrozenCLIP, PretokenizedPrompts, class_prompt_tables, image_conditioned_ctx, register_class_tables
from .per_image_text import PerImageTextCLIP
from .trainer import MVLPT, TrainerX, refuse_wide_heads


class PromptLearner(nn.Module):
    """trainers/cocoop.py:62-161.  ``clip_model`` is a :class:`FrozenCLIP`; ``pretokenized`` optionally gives the token ids."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        n_cls = len(classnames)
        n_ctx = cfg.TRAINER.COCOOP.N_CTX
        ctx_init = cfg.TRAINER.COCOOP.CTX_INIT
        dtype = clip_model.dtype                                                  # fp32 masters (module docstring)
        arch = clip_model.arch
        ctx_dim = arch.transformer_width                                          # ln_final.weight.shape[0]
        vis_dim = arch.embed_dim                                                  # visual.output_dim
        clip_imsize, cfg_imsize = arch.image_resolution, cfg.INPUT.SIZE[0]
        assert cfg_imsize == clip_imsize, f"cfg_imsize ({cfg_imsize}) must equal to clip_imsize ({clip_imsize})"

        ctx_vectors, self.meta_net, prompt_prefix, n_ctx = image_conditioned_ctx(    # :76-100
            clip_model, n_ctx, ctx_init, ctx_dim, vis_dim, dtype)
        self.ctx = nn.Parameter(ctx_vectors)

        self.n_ctx = n_ctx
        tables = class_prompt_tables(clip_model, classnames, pretokenized, prompt_prefix, cut=False)     # :105-111
        # construct_prompts (:125-145) is cat([prefix, ctx, suffix]): the "end" layout of the HIP text tower
        register_class_tables(self, n_cls, tables, n_ctx, "end")

    def forward(self, im_features):
        """:147-161 up to the shifted contexts [B, n_ctx, ctx_dim]; the prompts themselves are assembled by the HIP tower."""
        bias = self.meta_net(im_features).unsqueeze(1)       # (batch, 1, ctx_dim)
        return self.ctx.unsqueeze(0) + bias                  # (batch, n_ctx, ctx_dim)


class _CoCoOpLossFn(torch.autograd.Function):
    """Text side + head + cross-entropy of one CoCoOp training step as ONE autograd node.  Each chunk of images runs text
    forward over full ranges (saved) -> ranged logits -> cross-entropy -> ranged logits backward -> text backward straight away, so
    only one chunk's activations are alive.  Returns the mean loss over the batch; the backward hands out d loss / d ctx_shifted."""

    @staticmethod
    def forward(fctx, model: "CustomCLIP", img, ctx_shifted, label):
        eng = model.engine
        B = ctx_shifted.shape[0]
        lo, hi = model.full_ranges(B)
        chunks = model.chunks(lo, hi, model.text_len(ctx_shifted), save_for_bwd=True)
        dctx = torch.empty_like(ctx_shifted)
        loss = torch.zeros(1, device=ctx_shifted.device, dtype=torch.float32)
        ncorrect = torch.zeros(1, device=ctx_shifted.device, dtype=torch.float32)
        for g0, g1, _ in chunks:
            logits = model.chunk_logits(img, ctx_shifted, lo, hi, g0, g1, save=True)
            lc, dl, nc = eng.cross_entropy(logits, label[g0:g1], need_grad=True)
            if g1 - g0 != B:
                w = (g1 - g0) / B                            # the chunk's cross-entropy is a mean over its own images
                dl.mul_(w)
                lc = lc * w
            dctx[g0:g1] = eng.text_bwd(eng.logits_ranged_bwd(dl, need_img=False, need_txt=True)[1])
            loss += lc
            ncorrect += nc
        model.last_chunks = len(chunks)
        model.last_ncorrect = ncorrect
        fctx.save_for_backward(dctx)
        return loss.squeeze(0)

    @staticmethod
    def backward(fctx, g):
        (dctx,) = fctx.saved_tensors
        return None, None, dctx * g, None


class CustomCLIP(PerImageTextCLIP):
    """trainers/cocoop.py:164-194."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        self.prompt_learner = PromptLearner(cfg, classnames, clip_model, pretokenized)
        self._init_engine_side(cfg, clip_model)

    @torch.no_grad()
    def image_contexts(self, image) -> torch.Tensor:
        """ctx + meta_net(image features) [B, n_ctx, ctx_dim]: the contexts the text tower sees for these images (:178, :147-161).
        The prompt-free image tower keeps nothing for a backward on this route, so the call disturbs no pending backward."""
        img = self.engine.image_fwd(image.to(self.clip_model.device), None, None, save_for_bwd=False)
        return self.prompt_learner(img / img.norm(dim=-1, keepdim=True))

    def forward(self, image, label=None):
        """CE loss when `prompt_learner.training` (trainers/cocoop.py:191-192), the [B, n_cls] logits otherwise."""
        img = self.engine.image_fwd(image, None, None, save_for_bwd=False)          # frozen, prompt-free image tower
        imf = img / img.norm(dim=-1, keepdim=True)                                   # :178 (meta_net's input)
        if self.prompt_learner.training:
            if label is None:
                raise ValueError("CoCoOp training forward needs the labels (it returns the loss)")
            ctx_shifted = self.prompt_learner(imf)
            return _CoCoOpLossFn.apply(self, img, ctx_shifted, label)
        with torch.no_grad():
            ctx_shifted = self.prompt_learner(imf)
        return self.ranged_logits(img, ctx_shifted, *self.full_ranges(image.shape[0]))


class CoCoOp(MVLPT):
    """trainers/cocoop.py:197-315 on the HIP engine.  Data handling, test() and the loop are MVLPT's (Dassl's TrainerX)."""

    def check_cfg(self, cfg):
        """:199-200 accepts fp16 | fp32 | amp, with MVLPT.check_cfg's mapping; CustomCLIP then raises the default split_grad mode to
        split_all (split operands in every tower, see there), so all three run as PREC = "fp32" does."""
        assert cfg.TRAINER.COCOOP.PREC in ["fp16", "fp32", "amp"]

    def build_data_loader(self):
        super().build_data_loader()
        self.train_loader_x = self.dm.train_loader_x          # no image-tower look-ahead: CoCoOp's image features feed meta_net

    def build_model(self):
        cfg = self.cfg
        refuse_wide_heads(cfg, "CoCoOp")
        classnames = self.dm.dataset.classnames
        pretok = getattr(self.dm, "pretokenized", None)
        # fp16 / amp / fp32 all end in split_all (CustomCLIP raises the default mode); GRAD_PRECISION = "fast" keeps single operands
        prec = "split_all" if cfg.TRAINER.COCOOP.PREC == "fp32" else cfg.TRAINER.MVLPT.GRAD_PRECISION
        self.model = CustomCLIP(cfg, classnames, MVLPT.frozen_clip(self, prec), pretokenized=pretok)
        self.train_prompt_learner_only()                                # :220-241

    def forward_backward(self, batch):
        """:252-277: loss = model(image, label); zero_grad; backward; step."""
        image, label = self.parse_batch_train(batch)
        loss = self.model(image, label)
        self.model_backward_and_update(loss)
        loss_summary = {"loss": loss.detach()}            # device tensor: no host sync inside the step
        if (self.batch_idx + 1) == self.num_batches:
            self.update_lr()
        return loss_summary

    def parse_batch_train(self, batch):
        """:279-284"""
        return batch["img"].to(self.device), batch["label"].to(self.device)

    def parse_batch_test(self, batch):
        image, label = self.parse_batch_train(batch)
        return image, label, None

    def end_of_epoch_loop(self):
        TrainerX.end_of_epoch_loop(self)

    @torch.no_grad()
    def model_inference(self, input, task=None):
        return self.model(input)

    def interpret_images(self, images, topk: int = 5):
        """Nearest vocabulary words of ctx + meta_net(image features) per image (CustomCLIP.interpret_images); never called by the loop."""
        return self.model.interpret_images(images, topk)

    def load_state_dict_from_checkpoint(self, name, checkpoint):
        """:286-315 after the file read (MVLPT.load_model)."""
        print('Loading weights to {} (epoch = {})'.format(name, checkpoint.get("epoch")))
        super().load_state_dict_from_checkpoint(name, checkpoint)
