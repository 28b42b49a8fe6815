"""Zero-shot CLIP on the HIP engine: `ZeroshotCLIP` and `ZeroshotCLIP2` (prompt ensembling) of trainers/zsclip.py, the baseline row of
every prompt-tuning table.  Nothing is trained: `build_model` encodes the class prompts once, `model_inference` is the frozen image
tower plus the cosine head.

Prompts are `template.format(classname.replace("_", " "))` (trainers/zsclip.py:43, 90), tokenised by the shipped BPE tokenizer and fed to
`FrozenCLIP.encode_text` as token ids (mvlpt_text_encode_tokens: embedding lookup on the device, sequences trimmed to their EOT and
bucketed by length).  `ZeroshotCLIP2` runs ONE encode_text over all T x C prompts and one mvlpt_text_ensemble; the reference loops over
the templates.

Templates are configuration: `cfg.TRAINER.ZSCLIP.TEMPLATES`, a list of format strings (default ["a photo of a {}."]).  The package
ships no template table; the lists the reference uses are test data (tests/golden/zsclip_templates.json).
`ZeroshotCLIP` takes exactly one template, `ZeroshotCLIP2` any number >= 1.  Unlike the reference's `self.templates += [...]`
(trainers/zsclip.py:83), which grows a CLASS attribute on every build_model, the list is read from the config on every build and never
mutated.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from .model import FrozenCLIP
from .trainer import MVLPT, TrainerX


def build_prompts(templates: Sequence[str], classnames: Sequence[str]) -> List[str]:
    """Template-major prompt list: [t0 c0, t0 c1, ..., t1 c0, ...] (the order the reference loops in, trainers/zsclip.py:89-90)."""
    return [str(t).format(str(c).replace("_", " ")) for t in templates for c in classnames]


def read_templates(cfg, single: bool) -> List[str]:
    templates = list(cfg.TRAINER.ZSCLIP.TEMPLATES)
    if isinstance(cfg.TRAINER.ZSCLIP.TEMPLATES, str) or not templates or not all(isinstance(t, str) and "{}" in t for t in templates):
        raise ValueError("TRAINER.ZSCLIP.TEMPLATES must be a non-empty list of format strings containing '{}'")
    if single and len(templates) != 1:
        raise ValueError(f"ZeroshotCLIP takes exactly one template, got {len(templates)}; ZeroshotCLIP2 ensembles several")
    return templates


class ZeroshotCLIP(MVLPT):
    """trainers/zsclip.py:32-60.  Data handling and test() are MVLPT's (Dassl's TrainerX); there is no model to train or save."""

    single_template = True

    def check_cfg(self, cfg):
        read_templates(cfg, self.single_template)

    def build_data_loader(self):
        super().build_data_loader()
        self.train_loader_x = self.dm.train_loader_x          # nothing is trained: no look-ahead loader

    def build_model(self):
        cfg = self.cfg
        classnames = self.dm.dataset.classnames
        self.templates = read_templates(cfg, self.single_template)      # an instance attribute, rebuilt from the config every time
        # text tower: split operands unless "fast"
        clip_model: FrozenCLIP = MVLPT.frozen_clip(self, cfg.TRAINER.MVLPT.GRAD_PRECISION, include_token_embedding=True)
        prompts = build_prompts(self.templates, classnames)
        tokenized = clip_model.tokenizer.tokenize(prompts, clip_model.context_length)
        T, C = len(self.templates), len(classnames)
        feats = clip_model.encode_text(tokenized)                        # [T * C, embed], one call for every template
        self.text_features = clip_model.engine.text_ensemble(feats.view(T, C, -1))    # T = 1: x / |x| (:50)
        self.tokenized_prompts = tokenized
        self.clip_model = clip_model
        self.logit_scale_exp = float(clip_model.logit_scale.exp())
        self.bind_data(clip_model.engine)

    @torch.no_grad()
    def model_inference(self, image, task=None):
        """:55-60.  logits [B, n_cls] = exp(logit_scale) * <img / |img|, text_features> (mvlpt_logits_fwd, no mask)."""
        image_features = self.clip_model.encode_image(image)
        return self.clip_model.engine.logits_fwd(image_features, self.text_features, self.logit_scale_exp)

    def forward_backward(self, batch):
        raise RuntimeError("zero-shot CLIP has nothing to train: call test()")

    def end_of_epoch_loop(self):
        TrainerX.end_of_epoch_loop(self)

    def after_epoch(self):
        TrainerX.after_epoch(self)

    def load_model(self, directory, epoch=None):
        print("Note that load_model() is skipped: zero-shot CLIP has no trained parameters")


class ZeroshotCLIP2(ZeroshotCLIP):
    """Prompt ensembling (trainers/zsclip.py:63-99): the mean of the per-template unit features, normalised again."""

    single_template = False
