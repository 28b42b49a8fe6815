"""Minimal yacs-like config carrying the hot-path keys of the reference (train.py:105-169 `extend_cfg`,
configs/trainers/MVLPT/vit_b16.yaml) with the same names and defaults, so reference scripts' ``KEY VAL``
overrides map one-to-one.  Dassl/yacs are not available offline; this is only the key tree."""
from __future__ import annotations

from typing import Any, Iterable


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self) -> "CfgNode":
        return CfgNode({k: (v.clone() if isinstance(v, CfgNode) else v) for k, v in self.items()})

    def merge_from_list(self, opts: Iterable[Any]) -> None:
        """`KEY VAL KEY VAL …` overrides, as train.py:187."""
        opts = list(opts)
        assert len(opts) % 2 == 0, "override list must be KEY VAL pairs"
        for key, val in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = node[p]
            if parts[-1] not in node:
                raise KeyError(f"unknown config key {key}")
            old = node[parts[-1]]
            if isinstance(val, str) and not isinstance(old, str):
                if isinstance(old, bool):
                    val = val.lower() in ("1", "true", "yes")
                elif isinstance(old, list) and old and isinstance(old[0], str):
                    import json
                    val = [str(x) for x in json.loads(val)]      # a list of strings (TRAINER.ZSCLIP.TEMPLATES) comes as JSON
                elif key == "DATASET.SOURCES":
                    import json
                    val = [[str(x) for x in row] for row in json.loads(val)]      # JSON: [["task", "split.json or empty", "folder"], ...]
                elif isinstance(old, (list, tuple)):
                    val = type(old)(int(x) for x in val.strip("()[]").split(","))
                else:
                    val = type(old)(val)
            node[parts[-1]] = val


ACTIVATIONS = ("quick_gelu", "gelu")


def read_activation(cfg) -> str:
    """MODEL.BACKBONE.ACTIVATION (absent: "quick_gelu"), checked: the MLP activation every trainer hands to its engine."""
    act = cfg.MODEL.BACKBONE.get("ACTIVATION", "quick_gelu")
    if act not in ACTIVATIONS:
        raise ValueError(f"MODEL.BACKBONE.ACTIVATION = {act!r}: the accepted values are 'quick_gelu' and 'gelu'")
    return act


VISION_HEAD_WIDTHS = (64, 80, 96, 112, 128)


def read_vision_head_width(cfg) -> int:
    """MODEL.BACKBONE.VISION_HEAD_WIDTH, checked: the width of one head of a ViT image tower.  0 (or absent): the named backbone's own,
    64 for every CLIP ViT of the reference and 80 for "ViT-H/14".  A state dict does not say it (the reference computes heads =
    width // 64), so every trainer hands this value to the arch it builds from INIT_WEIGHTS."""
    w = cfg.MODEL.BACKBONE.get("VISION_HEAD_WIDTH", 0)
    if isinstance(w, bool) or not isinstance(w, int) or (w != 0 and w not in VISION_HEAD_WIDTHS):
        raise ValueError(f"MODEL.BACKBONE.VISION_HEAD_WIDTH = {w!r}: the accepted values are 0 (the backbone's own) and "
                         f"{', '.join(str(v) for v in VISION_HEAD_WIDTHS)}")
    if w == 0:
        from .weights import WIDE_HEAD_ARCHS
        arch = WIDE_HEAD_ARCHS.get(cfg.MODEL.BACKBONE.NAME)
        w = arch.vision_head_width if arch is not None else 64
    return w


def get_cfg_default() -> CfgNode:
    CN = CfgNode
    cfg = CN()
    cfg.SEED = 1
    cfg.OUTPUT_DIR = "./output"
    # ACTIVATION (not in the reference, whose clip/model.py:162-164 has QuickGELU compiled in): the MLP activation of both towers.
    # "quick_gelu": the archives clip.load downloads.  "gelu": a checkpoint with the same architecture and state-dict keys that was
    # trained with nn.GELU (the erf form); with the default its logits and gradients would come out of the wrong function without an error.
    # VISION_HEAD_WIDTH (not in the reference, whose clip/model.py:268 has heads = width // 64 compiled in): the width of one head of a ViT
    # image tower, 0 = the named backbone's own (64; "ViT-H/14": 80).  A wide-headed tower is frozen and forward-only (read_vision_head_width).
    cfg.MODEL = CN(BACKBONE=CN(NAME="ViT-B/16", ACTIVATION="quick_gelu", VISION_HEAD_WIDTH=0), INIT_WEIGHTS="")
    # TRANSFORMS and the parameters of its augmentations: Dassl's names and defaults (mvlpt_amd.transforms.build_device_transform; the
    # launcher's --transforms).  On the command line the list comes as JSON: INPUT.TRANSFORMS '["random_crop", "random_flip", "cutout"]'
    cfg.INPUT = CN(SIZE=(224, 224), TRANSFORMS=["random_resized_crop", "random_flip", "normalize"], COLORJITTER_B=0.4, COLORJITTER_C=0.4,
                   COLORJITTER_S=0.4, COLORJITTER_H=0.1, RGS_P=0.2, CROP_PADDING=4, CUTOUT_N=1, CUTOUT_LEN=16)
    # NUM_WORKERS: host threads of mvlpt_amd.data (file reads, header probes, Pillow decodes), at most 16.  Not in the reference:
    # RESIDENT_BYTES, the budget for splits kept decoded on the device (train, val, test in that order; 16 GiB covers ImageNet 16-shot,
    # 16 000 images of about 0.5 MB; 0: every split streams), and DECODE, "device" (mvlpt_jpeg_decode, Pillow for the files it does not
    # take) or "host" (Pillow for every file).
    cfg.DATALOADER = CN(TRAIN_X=CN(BATCH_SIZE=32), TEST=CN(BATCH_SIZE=100), NUM_WORKERS=8, RESIDENT_BYTES=16 * 2 ** 30, DECODE="device")
    # configs/trainers/MVLPT/vit_b16.yaml:15-22 + Dassl optimizer defaults
    cfg.OPTIM = CN(NAME="sgd", LR=0.002, MAX_EPOCH=200, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, SGD_DAMPNING=0.0,
                   SGD_NESTEROV=False, LR_SCHEDULER="cosine", WARMUP_EPOCH=1, WARMUP_TYPE="constant",
                   WARMUP_CONS_LR=1e-5, WARMUP_MIN_LR=1e-5,
                   # not in the reference: the one-launch HIP optimizer step over flat prompt buffers (mvlpt_amd.optim), opt-in
                   FUSED=False)
    cfg.TRAIN = CN(PRINT_FREQ=5, CHECKPOINT_FREQ=0)
    # Dassl's names and defaults (a run without evaluation data sets NO_TEST True).  PER_CLASS_RESULT / COMPUTE_CMAT: the per-class table
    # and the confusion matrix (OUTPUT_DIR/cmat.pt) of Dassl's Classification evaluator (mvlpt_amd.evaluator).  DEVICE_METRICS (not in the
    # reference): MVLPT.test finishes its figures from device counters whenever the logits are on a GPU; False keeps the host route.
    cfg.TEST = CN(FINAL_MODEL="last_step", SPLIT="test", NO_TEST=False, PER_CLASS_RESULT=False, COMPUTE_CMAT=False, DEVICE_METRICS=True)
    # ACT_CKPT (train.py:164, trainers/mvlpt.py:119-121): segments of the text tower's activation checkpointing; the three CustomCLIP
    # classes set it on their engine (Engine.set_text_act_ckpt).  1: every block's activations are saved.  It applies with or without
    # CUT_CONTEXTLEN (the reference: only with it) and changes memory and time, never a value.
    cfg.TRAINER = CN(NAME="MVLPT", CUT_CONTEXTLEN=False, ACT_CKPT=1)
    cfg.TRAINER.MVLPT = CN(
        PREC="fp16", PROJECT_METHOD="transformer", PROJECT_DIM=128,
        VPT=CN(N_CTX=0, CSC=False, CTX_INIT="", DROPOUT=0.0, PROJECT=-1, DEEP=True),
        # N_DEEP (not in the reference): deep language prompting, the text-side twin of VPT.DEEP.  The hidden states at the context
        # positions in front of text blocks 1 .. N_DEEP are replaced by learned rows (prompt_learner.ctx_deep [N_DEEP, n_ctx, width]);
        # with VPT.DEEP and PROJECT_METHOD "identity" beside it this is MaPLe's "independent V-L prompting".  0: off.  Needs
        # N_CTX > 0 and a generic context (no CSC), at most text_layers - 1; refused with the UPT projection and COCOOP.N_CTX != 0.
        COOP=CN(N_CTX=0, CSC=False, CTX_INIT="", CLASS_TOKEN_POSITION="middle", N_DEEP=0),
        COCOOP=CN(N_CTX=0, CTX_INIT="", PREC="fp16"),
        # not in the reference: MFMA input type of the MI355X towers
        COMPUTE_DTYPE="fp16",
        # not in the reference: "split_grad" (default: hi+lo operand pairs (GEMMs and attention) in towers that carry a
        # gradient: prompt gradients within 1e-3 of the fp32 CPU path) | "fast" (single 16-bit operands, ~4e-3)
        GRAD_PRECISION="split_grad",
        # not in the reference: compute the NEXT batch's image features underneath the current text-tower backward when
        # the method has no visual prompts (TrainerX.run_epoch reads the loader one batch ahead)
        STEP_PIPELINING=True,
        # not in the reference: (stop_block, cu_cap).  With step pipelining, the entry and blocks [0, stop_block) of the NEXT batch's image
        # tower are enqueued before this step's forward, on grids capped at cu_cap compute units (0: uncapped), beside the text forward;
        # the rest of the tower follows behind the cross-entropy as before.  (0, 0): the tower in one piece behind the cross-entropy.
        # Inert (one piece) with visual prompts, CoCoOp, a class-sharded text tower, a CU partition, the towers on one stream, and on
        # towers with fewer than stop_block + 1 blocks.  (6, 192): the headline step -1.2 % .. -2.7 % depending on the box (profiles/r07_prefetch_split_sweep.txt);
        # results are bit-identical either way.  MVLPT_PREFETCH_SPLIT=k:c overrides it (tools).
        PREFETCH_SPLIT=(6, 192),
        # the backbones (MODEL.BACKBONE.NAME) PREFETCH_SPLIT applies to; every other tower runs in one piece.  Measured: ViT-B/16 -2.1 % at
        # B = 256 and at B = 128, but ViT-B/32 (B = 256) +2.1 % and ViT-L/14 (B = 128) +1.0 % with the same setting.  (): every backbone.
        PREFETCH_SPLIT_TOWERS=("ViT-B/16",),
        # not in the reference: the text backward processes only the positions up to the largest EOT of the class table (the rows
        # behind a sequence's EOT carry an exactly zero gradient: Engine.set_text_grad_len).  The forward still evaluates every
        # position and every result keeps its bits; False runs the backward over all positions (A/B runs).
        TEXT_GRAD_TO_EOT=True,
        # not in the reference: with a generic context the leading positions of every class prompt (SOS and the context rows in
        # front of the class name: 1 + n_ctx/2 for "middle", 1 + n_ctx for "end") are the same rows in every class; the text tower
        # evaluates them once and its backward carries their gradient summed over the classes (Engine.set_text_shared_prefix).
        # The features keep their bits, dctx of those positions changes at rounding level; False evaluates them per class (A/B runs).
        TEXT_SHARED_PREFIX=True,
    )
    # trainers/cocoop.py's own keys (train.py:125-128), read by mvlpt_amd.cocoop (--trainer CoCoOp)
    cfg.TRAINER.COCOOP = CN(N_CTX=16, CTX_INIT="", PREC="fp16")
    # mvlpt_amd.zsclip (--trainer ZeroshotCLIP / ZeroshotCLIP2).  Not a reference key: the reference picks its templates from tables in
    # its own source by DATASET.NAME; here they are configuration.  ZeroshotCLIP takes exactly one, ZeroshotCLIP2 any number >= 1.
    cfg.TRAINER.ZSCLIP = CN(TEMPLATES=["a photo of a {}."])
    # mvlpt_amd.tpt (--trainer TPT): test-time prompt tuning (Shu et al., NeurIPS 2022), evaluation only.  Per test image N_VIEWS views
    # (view 0 the test view), the k = max(1, int(N_VIEWS * SELECTION_P)) most confident are kept, STEPS AdamW steps at LR on the image's
    # own copy of the context minimise the entropy of their averaged prediction.  The context starts from TRAINER.MVLPT.COOP (N_CTX /
    # CTX_INIT / CLASS_TOKEN_POSITION, e.g. with a CoOp checkpoint) when COOP.N_CTX != 0, else from N_CTX / CTX_INIT here, class at the end.
    cfg.TRAINER.TPT = CN(N_VIEWS=64, SELECTION_P=0.1, STEPS=1, LR=5e-3, N_CTX=4, CTX_INIT="a photo of a", PREC="fp16")
    # mvlpt_amd.tip_adapter (--trainer TipAdapter): Tip-Adapter (Zhang et al., ECCV 2022), zero-shot CLIP plus a key-value cache of the
    # few-shot features, with the published names in upper case.  AUGMENT_EPOCH passes over the few-shot set build the cache; INIT_ALPHA /
    # INIT_BETA hold until SEARCH_HP replaces them by the best point of the SEARCH_STEP grid over (0.1, SEARCH_SCALE) (beta first);
    # FINETUNE: Tip-Adapter-F, TRAIN_EPOCH epochs of AdamW(LR, EPS) on the cache keys.  The text classifier is TRAINER.ZSCLIP's.
    cfg.TRAINER.TIP = CN(AUGMENT_EPOCH=10, INIT_ALPHA=1.0, INIT_BETA=5.5, SEARCH_HP=True, SEARCH_SCALE=[7.0, 3.0], SEARCH_STEP=[200, 20],
                         FINETUNE=False, TRAIN_EPOCH=20, LR=1e-3, EPS=1e-4)
    # SOURCES (not in the reference, which has one reader module per dataset): [task name, CoOp split file or "", image folder] per dataset;
    # non-empty, a trainer that is given no data manager builds mvlpt_amd.data.DeviceDataManager from it.  On the command line as JSON.
    # SUBSAMPLE_CLASSES: all | base | new (train.py:117).
    cfg.DATASET = CN(NAME="synthetic", COOP=True, MULTITASK=False, MULTITASK_LABEL_PERTASK=False,
                     MULTITASK_EVALKEY="average", NUM_SHOTS=16, SOURCES=[], SUBSAMPLE_CLASSES="all")
    return cfg
