"""TEST INFRASTRUCTURE — generates the zero-shot CLIP fixtures under tests/golden/ from the REAL reference (trainers/zsclip.py).

Run where the reference tree is available (see oracle/ref_shim.py); the tests only read the files it writes:

    python tools/make_zsclip_golden.py

The reference's `ZeroshotCLIP` / `ZeroshotCLIP2` (trainers/zsclip.py:32-99) are instantiated WITHOUT Dassl's constructor (object.__new__
plus the three attributes build_model reads: cfg, dm, device), `load_clip_to_cpu` in the module's namespace is replaced by a
`clip.model.CLIP` whose fp32 weights come from our deterministic generator (oracle.make_golden.build_ref_clip, used read-only), and
`build_model` / `model_inference` run on the CPU.  Inputs and outputs are stored as data:
  zsclip_templates.json        the reference's per-dataset templates, its 7 selected and its 80 ImageNet templates (lists of strings)
  tiny_zsclip.npz              tiny arch, 5 classes, the dataset's one template, B 3: clip.tokenize ids, images, text_features, logits
  tiny_zsclip_ensemble.npz     the same classes, the 7 selected templates plus the dataset's own (T = 8)
  full_vitb16_zsclip.npz       ViT-B/16, 10 classes, T = 8, B 2: outputs only, weights and images regenerated from the stored seeds
Every file also holds the per-template un-normalised features (clip_model.encode_text per template), from which the stored
text_features follow by the ensemble formula (tests/test_zsclip_host.py checks that in float64).
"""
from __future__ import annotations

import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import ARCHS, CLASSNAMES, build_ref_clip  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TINY_SEED, FULL_SEED = 1, 2          # oracle/make_golden.py: the frozen weights of tiny_clip.npz / the full_* cases
DATASET = "OxfordPets"               # a dataset whose own template differs from the selected seven


def run_case(zs, clip_mod, clip_model, *, name, trainer, image_size, classnames, B, case_seed, store_inputs=True):
    ns = SimpleNamespace
    cls = getattr(zs, trainer)
    if trainer == "ZeroshotCLIP2":
        # the reference appends to a CLASS attribute on every build_model (trainers/zsclip.py:83): start from its own list each time
        cls.templates = list(zs.IMAGENET_TEMPLATES_SELECT)
    tr = object.__new__(cls)
    tr.cfg = ns(MODEL=ns(BACKBONE=ns(NAME="synthetic")), DATASET=ns(NAME=DATASET))
    tr.dm = ns(dataset=ns(classnames=list(classnames)))
    tr.device = torch.device("cpu")
    zs.load_clip_to_cpu = lambda cfg: clip_model
    g = torch.Generator().manual_seed(case_seed + 1000)
    image = torch.randn(B, 3, image_size, image_size, generator=g)
    with torch.no_grad():
        tr.build_model()
        logits = tr.model_inference(image)
        templates = [zs.CUSTOM_TEMPLATES[DATASET]] if trainer == "ZeroshotCLIP" else list(cls.templates)
        tokens, per_template = [], []
        for temp in templates:
            ids = torch.cat([clip_mod.tokenize(temp.format(c.replace("_", " "))) for c in classnames])
            tokens.append(ids)
            per_template.append(clip_model.encode_text(ids))
    d = {
        "classnames": np.array(list(classnames)), "templates": np.array(templates), "dataset_name": np.array(DATASET),
        "trainer": np.array(trainer),
        "tokenized_prompts": torch.cat(tokens).numpy().astype(np.int64),            # [T * C, 77], template-major
        "text_features_per_template": torch.stack(per_template).numpy(),             # [T, C, e], un-normalised
        "text_features": tr.text_features.numpy(),                                   # [C, e], what the trainer keeps
        "out_logits": logits.numpy(),
        "logit_scale": clip_model.logit_scale.detach().numpy(),
        "case_seed": np.int64(case_seed),
    }
    if store_inputs:
        d["image"] = image.numpy()
    else:
        d["image_seed"] = np.int64(case_seed + 1000)
        d["image_batch"] = np.int64(B)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(f"[golden] {name}: T {len(templates)} text_features {tuple(tr.text_features.shape)} logits {tuple(logits.shape)}")


def main():
    ref_shim.install()
    cm = importlib.import_module("clip.model")
    clip_mod = importlib.import_module("clip.clip")
    zs = importlib.import_module("trainers.zsclip")
    with open(os.path.join(OUT, "zsclip_templates.json"), "w") as f:
        json.dump({"note": "prompt templates trainers/zsclip.py and trainers/imagenet_templates.py use (data: lists of strings)",
                   "per_dataset": dict(zs.CUSTOM_TEMPLATES), "imagenet_select": list(zs.IMAGENET_TEMPLATES_SELECT),
                   "imagenet": list(zs.IMAGENET_TEMPLATES)}, f, indent=1)
    names = [c.replace(" ", "_") for c in CLASSNAMES]      # underscores, as Dassl class names carry them (replaced at :43 / :90)
    arch = ARCHS["tiny"]
    clip_model, _ = build_ref_clip(cm, arch, TINY_SEED)
    common = dict(image_size=arch.image_resolution, classnames=names[:5], B=3)
    run_case(zs, clip_mod, clip_model, name="tiny_zsclip", trainer="ZeroshotCLIP", case_seed=61, **common)
    run_case(zs, clip_mod, clip_model, name="tiny_zsclip_ensemble", trainer="ZeroshotCLIP2", case_seed=62, **common)
    arch = ARCHS["ViT-B/16"]
    clip_model, _ = build_ref_clip(cm, arch, FULL_SEED)
    run_case(zs, clip_mod, clip_model, name="full_vitb16_zsclip", trainer="ZeroshotCLIP2", image_size=224, classnames=names[:10], B=2,
             case_seed=63, store_inputs=False)


if __name__ == "__main__":
    main()
