"""CoCoOp (trainers/cocoop.py) on the HIP engine: image-conditioned prompts, `--trainer CoCoOp`.

Same class names, constructor arguments and ``prompt_learner.state_dict()`` keys as the reference (``ctx``,
``meta_net.linear{1,2}.{weight,bias}``, ``token_prefix``, ``token_suffix``), so CoCoOp checkpoints interoperate.

Every image g gets its own context ``ctx + meta_net(img_g / |img_g|)``, so the text tower runs over B x n_cls sequences per
step.  The reference loops over the images in Python (trainers/cocoop.py:184-189) and trains at batch size 1; here the
whole batch (or the largest chunk of it whose workspace fits ``CustomCLIP.max_text_workspace_bytes``) is ONE grouped tower
(mvlpt_text_fwd_grouped: the [n_cls, ...] prefix / suffix / layout tables are read per group, never copied) followed by the
grouped cosine head (mvlpt_logits_grouped_fwd / _bwd) and the existing cross-entropy kernel.  ``meta_net`` and
``ctx + bias`` (a few thousand FLOPs per image, trainable) stay on torch autograd, as the UPT projection does.

Deviations: parameters are fp32 masters for every PREC (the reference halves ``meta_net`` under fp16); the
prompt learner's ``forward`` returns the shifted contexts [B, n_ctx, ctx_dim] — the prompt assembly is a HIP kernel.
"""
from __future__ import annotations

import os.path as osp
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from . import distributed as dist_utils
from .model import FrozenCLIP, PretokenizedPrompts, _text_inputs, apply_text_act_ckpt, build_prompt_layout
from .trainer import MVLPT, TrainerX, build_lr_scheduler, build_optimizer, load_pretrained_weights
from .weights import get_arch, make_state_dict

# Workspace budget of the CoCoOp text tower (not a reference key).  A chunk is the largest number of images whose grouped
# text tower fits it (mvlpt_text_workspace_bytes).  ViT-B/16 with 100 classes needs 1.67 GiB per image for a training step.
DEFAULT_MAX_TEXT_WORKSPACE_BYTES = 16 << 30
# sequences per grouped tower: the attention launches put the sequence index on grid.y
MAX_SEQUENCES_PER_TOWER = 32768


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

        if ctx_init:                                                              # :76-84
            ctx_init = ctx_init.replace("_", " ")
            n_ctx = len(ctx_init.split(" "))
            ids = clip_model.tokenizer.tokenize(ctx_init)
            with torch.no_grad():
                ctx_vectors = clip_model.token_embedding(ids)[0, 1:1 + n_ctx, :].to(dtype)
            prompt_prefix = ctx_init
        else:                                                                     # :85-89
            ctx_vectors = torch.empty(n_ctx, ctx_dim, dtype=dtype)
            nn.init.normal_(ctx_vectors, std=0.02)
            prompt_prefix = " ".join(["X"] * n_ctx)
        self.ctx = nn.Parameter(ctx_vectors)
        self.meta_net = nn.Sequential(OrderedDict([                               # :96-100
            ("linear1", nn.Linear(vis_dim, vis_dim // 16)),
            ("relu", nn.ReLU(inplace=True)),
            ("linear2", nn.Linear(vis_dim // 16, ctx_dim)),
        ]))

        if pretokenized is not None:
            tokenized_prompts, name_lens = pretokenized.tokenized_prompts, pretokenized.name_lens
        else:                                                                     # :105-108
            tok = clip_model.tokenizer
            names = [name.replace("_", " ") for name in classnames]
            name_lens = [len(tok.encode(name)) for name in names]
            prompts = [prompt_prefix + " " + name + "." for name in names]
            tokenized_prompts = torch.cat([tok.tokenize(p, context_length=clip_model.context_length) for p in prompts])
        with torch.no_grad():
            embedding = clip_model.token_embedding(tokenized_prompts).to(dtype)
        # saved by save_model, dropped by load_model (:113-118)
        self.register_buffer("token_prefix", embedding[:, :1, :].contiguous())              # SOS
        self.register_buffer("token_suffix", embedding[:, 1 + n_ctx:, :].contiguous())      # CLS, EOS

        self.n_cls, self.n_ctx = n_cls, n_ctx
        self.tokenized_prompts = tokenized_prompts
        self.name_lens = list(name_lens)
        L = tokenized_prompts.shape[1]
        # construct_prompts (:125-145) is cat([prefix, ctx, suffix]): the "end" layout of the HIP text tower
        self.register_buffer("layout", build_prompt_layout(self.name_lens, n_ctx, L, "end"), persistent=False)
        self.register_buffer("eot", tokenized_prompts.argmax(dim=-1).to(torch.int32), persistent=False)
        self.max_eot = int(self.eot.max())

    def forward(self, im_features):
        """:147-161 up to the shifted contexts [B, n_ctx, ctx_dim]; the prompts themselves are assembled by the HIP tower."""
        bias = self.meta_net(im_features).unsqueeze(1)       # (batch, 1, ctx_dim)
        return self.ctx.unsqueeze(0) + bias                  # (batch, n_ctx, ctx_dim)


class _CoCoOpLossFn(torch.autograd.Function):
    """Text side + head + cross-entropy of one CoCoOp training step as ONE autograd node.  Each chunk of images runs grouped
    text forward (saved) -> grouped logits -> cross-entropy -> grouped logits backward -> text backward straight away, so only
    one chunk's activations are alive.  Returns the mean loss over the batch; the backward hands out d loss / d ctx_shifted."""

    @staticmethod
    def forward(fctx, model: "CustomCLIP", img, ctx_shifted, label):
        eng, pl = model.engine, model.prompt_learner
        suffix, layout = _text_inputs(model, pl, pl.n_ctx)
        B = ctx_shifted.shape[0]
        step = model.images_per_chunk(B, layout.shape[1], save_for_bwd=True)
        dctx = torch.empty_like(ctx_shifted)
        loss = torch.zeros(1, device=ctx_shifted.device, dtype=torch.float32)
        ncorrect = torch.zeros(1, device=ctx_shifted.device, dtype=torch.float32)
        for g0 in range(0, B, step):
            g1 = min(B, g0 + step)
            w = (g1 - g0) / B                                # the chunk's cross-entropy is a mean over its own images
            txt = eng.text_fwd_grouped(pl.token_prefix, suffix, ctx_shifted[g0:g1], layout, pl.eot, save_for_bwd=True)
            logits = eng.logits_grouped_fwd(img[g0:g1], txt, model.logit_scale_exp)
            lc, dl, nc = eng.cross_entropy(logits, label[g0:g1], need_grad=True)
            if g1 - g0 != B:
                dl.mul_(w)
                lc = lc * w
            dctx[g0:g1] = eng.text_bwd(eng.logits_grouped_bwd(dl))
            loss += lc
            ncorrect += nc
        model.last_chunks = -(-B // step)
        model.last_ncorrect = ncorrect
        fctx.save_for_backward(dctx)
        return loss.squeeze(0)

    @staticmethod
    def backward(fctx, g):
        (dctx,) = fctx.saved_tensors
        return None, None, dctx * g, None


class CustomCLIP(nn.Module):
    """trainers/cocoop.py:164-194."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        self.prompt_learner = PromptLearner(cfg, classnames, clip_model, pretokenized)
        self.tokenized_prompts = self.prompt_learner.tokenized_prompts
        self.clip_model = clip_model
        self.engine = clip_model.engine
        self.text_act_ckpt = apply_text_act_ckpt(cfg, self.engine)      # TRAINER.ACT_CKPT: images_per_chunk sees the smaller workspace
        self.logit_scale = clip_model.logit_scale
        self.logit_scale_exp = float(clip_model.logit_scale.exp())
        self.dtype = clip_model.dtype
        self.trim_text_to_eot = False        # mvlpt_amd.model.CustomCLIP's switch, same default
        self.max_text_workspace_bytes = DEFAULT_MAX_TEXT_WORKSPACE_BYTES
        # Precision: the image features are meta_net's input and every text row carries a gradient, so under the
        # default mode (split operands only in towers kept for a backward) the ViT-B/16 fixture's ctx / meta_net gradients land at
        # 0.9-1.3e-3 of the reference; with split operands in every tower (MVLPT_PREC_SPLIT_ALL) at <= 8.3e-4.  CoCoOp therefore
        # raises the engine's default mode to split_all ("fast", an explicit request for single operands, is left alone).
        if self.engine.precision == _lib.PREC_SPLIT_GRAD:
            self.engine.set_precision("split_all")
        self.last_chunks = 0
        self.last_ncorrect = None

    def images_per_chunk(self, B: int, L: int, save_for_bwd: bool) -> int:
        """Largest number of images (<= B) whose grouped text tower fits `max_text_workspace_bytes`; at least 1."""
        C = self.prompt_learner.n_cls
        lo, hi = 1, max(1, min(B, MAX_SEQUENCES_PER_TOWER // C))
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if self.engine.text_workspace_bytes(mid * C, L, save_for_bwd) <= self.max_text_workspace_bytes:
                lo = mid
            else:
                hi = mid - 1
        return lo

    @torch.no_grad()
    def _eval_logits(self, img, ctx_shifted):
        eng, pl = self.engine, self.prompt_learner
        suffix, layout = _text_inputs(self, pl, pl.n_ctx)
        B = ctx_shifted.shape[0]
        step = self.images_per_chunk(B, layout.shape[1], save_for_bwd=False)
        out = torch.empty(B, pl.n_cls, device=img.device, dtype=torch.float32)
        for g0 in range(0, B, step):
            g1 = min(B, g0 + step)
            txt = eng.text_fwd_grouped(pl.token_prefix, suffix, ctx_shifted[g0:g1], layout, pl.eot, save_for_bwd=False)
            out[g0:g1] = eng.logits_grouped_fwd(img[g0:g1], txt, self.logit_scale_exp)
        self.last_chunks = -(-B // step)
        return out

    @torch.no_grad()
    def image_contexts(self, image) -> torch.Tensor:
        """ctx + meta_net(image features) [B, n_ctx, ctx_dim]: the contexts the text tower sees for these images (:178, :147-161).
        The prompt-free image tower keeps nothing for a backward on this route, so the call disturbs no pending backward."""
        img = self.engine.image_fwd(image.to(self.clip_model.device), None, None, save_for_bwd=False)
        return self.prompt_learner(img / img.norm(dim=-1, keepdim=True))

    def interpret_images(self, images, topk: int = 5):
        """Nearest vocabulary words of every image's own contexts: [B][n_ctx] lists of (word, distance), B * n_ctx rows in ONE
        nearest-token call (mvlpt_amd.interpret)."""
        from .interpret import nearest_words
        return nearest_words(self.clip_model, self.image_contexts(images), topk)

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
        return self._eval_logits(img, ctx_shifted)


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
        classnames = self.dm.dataset.classnames
        pretok = getattr(self.dm, "pretokenized", None)
        sd = self._sd_arg
        if sd is None:
            sd = make_state_dict(get_arch(cfg.MODEL.BACKBONE.NAME), seed=cfg.SEED)
        # fp16 / amp / fp32 all end in split_all (CustomCLIP raises the default mode); GRAD_PRECISION = "fast" keeps single operands
        prec = "split_all" if cfg.TRAINER.COCOOP.PREC == "fp32" else cfg.TRAINER.MVLPT.GRAD_PRECISION
        clip_model = FrozenCLIP(sd, compute_dtype=cfg.TRAINER.MVLPT.COMPUTE_DTYPE, device=self.device, precision=prec)
        self.model = CustomCLIP(cfg, classnames, clip_model, pretokenized=pretok)
        for name, param in self.model.named_parameters():               # :220-225
            if "prompt_learner" not in name:
                param.requires_grad_(False)
        if cfg.MODEL.INIT_WEIGHTS:
            load_pretrained_weights(self.model.prompt_learner, cfg.MODEL.INIT_WEIGHTS)    # :233-234
        self.model.to(self.device)
        if self.world_size > 1:
            dist_utils.broadcast_parameters(self.model.prompt_learner)
        self.optim, self.sched = self.build_optim("prompt_learner", self.model.prompt_learner)   # :238-241
        self.scaler = None    # amp: the HIP backward scales its 16-bit activation gradients internally (MVLPT.check_cfg)

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

    def load_model(self, directory, epoch=None):
        """:286-315 (token_prefix / token_suffix are dropped: they come from the current class names)."""
        if not directory:
            print("Note that load_model() is skipped as no pretrained model is given")
            return
        model_file = "model-best.pth.tar" if epoch is None else "model.pth.tar-" + str(epoch)
        for name in self.get_model_names():
            path = osp.join(directory, name, model_file)
            if not osp.exists(path):
                raise FileNotFoundError('Model not found at "{}"'.format(path))
            ck = torch.load(path, map_location="cpu")
            self.load_state_dict_from_checkpoint(name, ck)

    def load_state_dict_from_checkpoint(self, name, checkpoint):
        """The part of load_model after the file read: `checkpoint` is a Dassl checkpoint dict (state_dict, epoch, ...)."""
        state_dict = dict(checkpoint["state_dict"])
        state_dict.pop("token_prefix", None)
        state_dict.pop("token_suffix", None)
        print('Loading weights to {} (epoch = {})'.format(name, checkpoint.get("epoch")))
        self._models[name].load_state_dict(state_dict, strict=False)
