"""Architecture table and deterministic synthetic frozen-CLIP weights.

Pretrained CLIP checkpoints cannot be downloaded here (clip/clip.py:41-70 needs network), and
neither parity nor throughput depends on trained values, so tests and `bench.py` use seeded
random weights with the reference's own initialisation scales (clip/model.py:209-217, 295-322)
under the reference's own ``state_dict`` key names.  The same function runs in the build
container (to feed the real reference when golden fixtures are generated) and on the GPU box.
"""
from __future__ import annotations

import hashlib
import math
from dataclasses import dataclass
from typing import Dict, Tuple, Union

import torch


@dataclass(frozen=True)
class ClipArch:
    name: str
    embed_dim: int
    image_resolution: int
    vision_layers: int
    vision_width: int
    vision_patch_size: int
    context_length: int
    vocab_size: int
    transformer_width: int
    transformer_heads: int
    transformer_layers: int
    # width of one image-tower head: 64 in every ViT of the reference (clip/model.py:268 computes heads = width // 64, so its
    # build_model cannot describe anything else); 80 in the ViT-H/14 family (width 1280 = 16 heads of 80)
    vision_head_width: int = 64

    @property
    def vision_heads(self) -> int:
        return self.vision_width // self.vision_head_width

    @property
    def grid(self) -> int:
        return self.image_resolution // self.vision_patch_size

    def ctor_args(self):
        """Positional arguments of clip.model.CLIP.__init__ (clip/model.py:240-253)."""
        return (self.embed_dim, self.image_resolution, self.vision_layers, self.vision_width,
                self.vision_patch_size, self.context_length, self.vocab_size,
                self.transformer_width, self.transformer_heads, self.transformer_layers)


ARCHS: Dict[str, ClipArch] = {
    "ViT-B/32": ClipArch("ViT-B/32", 512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    "ViT-B/16": ClipArch("ViT-B/16", 512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    "ViT-L/14": ClipArch("ViT-L/14", 768, 224, 24, 1024, 14, 77, 49408, 768, 12, 12),
    "ViT-L/14@336px": ClipArch("ViT-L/14@336px", 768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
    # test-size architecture: head_dim stays 64 as in every CLIP ViT (heads = width // 64)
    "tiny": ClipArch("tiny", 128, 32, 3, 128, 16, 77, 49408, 128, 2, 2),
}

# ViT backbones whose image tower has heads wider than 64: frozen, prompt-free and forward-only here (csrc/attention_wide.hip).  Kept
# apart from ARCHS as RESNET_ARCHS is: ARCHS stays the list of the backbones every trainer configuration runs on (and the reference builds).
WIDE_HEAD_ARCHS: Dict[str, ClipArch] = {
    # the ViT-H/14 family (LAION-2B, DFN, MetaCLIP, CLIPA): image tower 1280 = 16 heads of 80, text tower 1024 = 16 heads of 64, 24 layers
    "ViT-H/14": ClipArch("ViT-H/14", 1024, 224, 32, 1280, 14, 77, 49408, 1024, 16, 24, vision_head_width=80),
    # test-size architecture: 640 = 8 heads of 80 (the smallest multiple of 128 that 80 divides), 10 tokens
    "tiny-h": ClipArch("tiny-h", 128, 48, 3, 640, 16, 77, 49408, 128, 2, 2, vision_head_width=80),
}


@dataclass(frozen=True)
class ResNetClipArch:
    """A CLIP whose image tower is ModifiedResNet (clip/model.py:94-150): `vision_layers` is the tuple of blocks per stage and
    `vision_width` the stem width; the attention pool runs over 32 * width channels."""
    name: str
    embed_dim: int
    image_resolution: int
    vision_layers: Tuple[int, int, int, int]
    vision_width: int
    context_length: int
    vocab_size: int
    transformer_width: int
    transformer_heads: int
    transformer_layers: int
    vision_patch_size = None      # what clip.model.CLIP takes for a ResNet

    @property
    def vision_heads(self) -> int:  # clip/model.py:258
        return self.vision_width * 32 // 64

    @property
    def grid(self) -> int:
        return self.image_resolution // 32

    @property
    def pool_width(self) -> int:
        return self.vision_width * 32

    def ctor_args(self):
        """Positional arguments of clip.model.CLIP.__init__ (clip/model.py:240-253)."""
        return (self.embed_dim, self.image_resolution, tuple(self.vision_layers), self.vision_width, None, self.context_length,
                self.vocab_size, self.transformer_width, self.transformer_heads, self.transformer_layers)


AnyArch = Union[ClipArch, ResNetClipArch]

# Kept apart from ARCHS: that table is the list of ViT backbones (tools that need a ViT check membership in it).
RESNET_ARCHS: Dict[str, ResNetClipArch] = {
    "RN50": ResNetClipArch("RN50", 1024, 224, (3, 4, 6, 3), 64, 77, 49408, 512, 8, 12),
    "RN101": ResNetClipArch("RN101", 512, 224, (3, 4, 23, 3), 64, 77, 49408, 512, 8, 12),
    # test-size architecture: channels 8 .. 512, a 2 x 2 attention pool (5 tokens), every stage and both block kinds present
    "tiny-rn": ResNetClipArch("tiny-rn", 128, 64, (1, 2, 1, 1), 16, 77, 49408, 128, 2, 2),
}


def is_resnet(arch) -> bool:
    return isinstance(arch, ResNetClipArch)


def get_arch(name: str) -> AnyArch:
    """The architecture of a backbone name (cfg.MODEL.BACKBONE.NAME), ViT or ResNet."""
    if name in ARCHS:
        return ARCHS[name]
    if name in WIDE_HEAD_ARCHS:
        return WIDE_HEAD_ARCHS[name]
    if name in RESNET_ARCHS:
        return RESNET_ARCHS[name]
    raise KeyError(f"unknown backbone {name!r}: known are {sorted(ARCHS) + sorted(WIDE_HEAD_ARCHS) + sorted(RESNET_ARCHS)}")



def arch_from_state_dict(sd: Dict[str, torch.Tensor], name: str = "custom", vision_head_width: int = 64) -> AnyArch:
    """Same shape inference as clip.model.build_model (clip/model.py:395-418).  The head width of a ViT image tower is not in a state
    dict (the reference assumes 64): `vision_head_width` says it (MODEL.BACKBONE.VISION_HEAD_WIDTH; 80 for a ViT-H/14 checkpoint)."""
    tw = sd["ln_final.weight"].shape[0]
    tl = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks")})
    vocab = sd["token_embedding.weight"].shape[0] if "token_embedding.weight" in sd else 49408
    if "visual.layer1.0.conv1.weight" in sd:
        counts = tuple(len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{b}.")}) for b in (1, 2, 3, 4))
        vw = sd["visual.layer1.0.conv1.weight"].shape[0]
        grid = round((sd["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
        return ResNetClipArch(name, sd["text_projection"].shape[1], grid * 32, counts, vw, sd["positional_embedding"].shape[0],
                              vocab, tw, tw // 64, tl)
    vw = sd["visual.conv1.weight"].shape[0]
    vl = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    ps = sd["visual.conv1.weight"].shape[-1]
    grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    if vision_head_width <= 0 or vw % vision_head_width:
        raise ValueError(f"the image tower's width {vw} is not a multiple of the head width {vision_head_width} "
                         "(MODEL.BACKBONE.VISION_HEAD_WIDTH)")
    return ClipArch(name, sd["text_projection"].shape[1], ps * grid, vl, vw, ps,
                    sd["positional_embedding"].shape[0], vocab, tw, tw // 64, tl, vision_head_width=vision_head_width)


def _randn(name: str, seed: int, shape, std: float, fp16_exact: bool = False) -> torch.Tensor:
    h = int.from_bytes(hashlib.sha256(f"{seed}:{name}".encode()).digest()[:7], "little")
    g = torch.Generator(device="cpu").manual_seed(h)
    w = torch.randn(tuple(shape), generator=g, dtype=torch.float32) * std
    # Real CLIP checkpoints store conv/linear/attention/projection tensors in fp16 (clip/model.py:371-392
    # convert_weights; "CLIP's default precision is fp16", trainers/mvlpt.py:849) and the fp32/amp modes only
    # up-cast them: such values are exactly representable in fp16.  Mirror that so that parity measures the
    # kernels' arithmetic and not a weight quantisation real checkpoints never undergo.
    return w.half().float() if fp16_exact else w


def make_state_dict(arch: AnyArch, seed: int = 0, *, include_token_embedding: bool = False,
                    randomize_affine: bool = True) -> Dict[str, torch.Tensor]:
    """fp32 CPU tensors keyed like clip.model.CLIP.state_dict().  With ``randomize_affine`` the
    LayerNorm scales/shifts and all biases are non-trivial so a dropped bias or γ shows in parity."""
    sd: Dict[str, torch.Tensor] = {}

    def affine(prefix: str, d: int):
        if randomize_affine:
            sd[prefix + ".weight"] = 1.0 + _randn(prefix + ".weight", seed, (d,), 0.1)
            sd[prefix + ".bias"] = _randn(prefix + ".bias", seed, (d,), 0.1)
        else:
            sd[prefix + ".weight"] = torch.ones(d)
            sd[prefix + ".bias"] = torch.zeros(d)

    def bias(name: str, d: int):
        sd[name] = _randn(name, seed, (d,), 0.02, True) if randomize_affine else torch.zeros(d)

    def tower(prefix: str, width: int, layers: int, init_width: int, init_layers: int):
        # clip/model.py:312-319 uses the TEXT transformer's width/layers for the text tower;
        # the vision tower keeps nn defaults there — we use the same formula with its own dims.
        proj_std = (init_width ** -0.5) * ((2 * init_layers) ** -0.5)
        attn_std = init_width ** -0.5
        fc_std = (2 * init_width) ** -0.5
        for l in range(layers):
            p = f"{prefix}resblocks.{l}."
            sd[p + "attn.in_proj_weight"] = _randn(p + "attn.in_proj_weight", seed, (3 * width, width), attn_std, True)
            bias(p + "attn.in_proj_bias", 3 * width)
            sd[p + "attn.out_proj.weight"] = _randn(p + "attn.out_proj.weight", seed, (width, width), proj_std, True)
            bias(p + "attn.out_proj.bias", width)
            affine(p + "ln_1", width)
            sd[p + "mlp.c_fc.weight"] = _randn(p + "mlp.c_fc.weight", seed, (4 * width, width), fc_std, True)
            bias(p + "mlp.c_fc.bias", 4 * width)
            sd[p + "mlp.c_proj.weight"] = _randn(p + "mlp.c_proj.weight", seed, (width, 4 * width), proj_std, True)
            bias(p + "mlp.c_proj.bias", width)
            affine(p + "ln_2", width)

    def vit_tower():
        vw, p = arch.vision_width, arch.vision_patch_size
        scale = vw ** -0.5
        sd["visual.conv1.weight"] = _randn("visual.conv1.weight", seed, (vw, 3, p, p), (3 * p * p) ** -0.5, True)
        sd["visual.class_embedding"] = _randn("visual.class_embedding", seed, (vw,), scale)
        sd["visual.positional_embedding"] = _randn("visual.positional_embedding", seed, (arch.grid ** 2 + 1, vw), scale)
        affine("visual.ln_pre", vw)
        tower("visual.transformer.", vw, arch.vision_layers, vw, arch.vision_layers)
        affine("visual.ln_post", vw)
        sd["visual.proj"] = _randn("visual.proj", seed, (vw, arch.embed_dim), scale, True)

    def resnet_tower():
        """ModifiedResNet under the reference's key names.  The scales keep every block's output rms near 1 through 33 blocks, so
        that fp16 activations neither overflow nor lose the residual branch: conv weights N(0, 2 / fan_in); BatchNorm weight
        1 +- 0.1, bias and running mean 0.1 N, running variance in [1, 1.2); bn3 (the last of a block) 0.25 (1 +- 0.1) — the
        reference's zero init would hide the residual branch from a parity test, 1 lets the rms grow with depth."""
        def conv(name: str, cout: int, cin: int, k: int):
            sd[name + ".weight"] = _randn(name + ".weight", seed, (cout, cin, k, k), (2.0 / (cin * k * k)) ** 0.5, True)

        def bn(name: str, c: int, gain: float = 1.0):
            sd[name + ".weight"] = gain * (1.0 + _randn(name + ".weight", seed, (c,), 0.1))
            sd[name + ".bias"] = _randn(name + ".bias", seed, (c,), 0.1)
            sd[name + ".running_mean"] = _randn(name + ".running_mean", seed, (c,), 0.1)
            h = int.from_bytes(hashlib.sha256(f"{seed}:{name}.running_var".encode()).digest()[:7], "little")
            sd[name + ".running_var"] = 1.0 + 0.2 * torch.rand(c, generator=torch.Generator(device="cpu").manual_seed(h))
            sd[name + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64)

        w = arch.vision_width
        for i, (cout, cin) in enumerate(((w // 2, 3), (w // 2, w // 2), (w, w // 2)), start=1):
            conv(f"visual.conv{i}", cout, cin, 3)
            bn(f"visual.bn{i}", cout)
        inplanes = w
        for st, blocks in enumerate(arch.vision_layers):
            planes = w << st
            for i in range(blocks):
                q = f"visual.layer{st + 1}.{i}."
                stride = 2 if (i == 0 and st > 0) else 1
                conv(q + "conv1", planes, inplanes, 1); bn(q + "bn1", planes)
                conv(q + "conv2", planes, planes, 3); bn(q + "bn2", planes)
                conv(q + "conv3", planes * 4, planes, 1); bn(q + "bn3", planes * 4, 0.25)
                if stride > 1 or inplanes != planes * 4:
                    conv(q + "downsample.0", planes * 4, inplanes, 1); bn(q + "downsample.1", planes * 4)
                inplanes = planes * 4
        E = arch.pool_width
        sd["visual.attnpool.positional_embedding"] = _randn("visual.attnpool.positional_embedding", seed, (arch.grid ** 2 + 1, E), E ** -0.5)
        for n, out in (("q", E), ("k", E), ("v", E), ("c", arch.embed_dim)):
            sd[f"visual.attnpool.{n}_proj.weight"] = _randn(f"visual.attnpool.{n}_proj.weight", seed, (out, E), E ** -0.5, True)
            sd[f"visual.attnpool.{n}_proj.bias"] = _randn(f"visual.attnpool.{n}_proj.bias", seed, (out,), 0.02)

    if isinstance(arch, ResNetClipArch):
        resnet_tower()
    else:
        vit_tower()

    tw = arch.transformer_width
    tower("transformer.", tw, arch.transformer_layers, tw, arch.transformer_layers)
    if include_token_embedding:
        sd["token_embedding.weight"] = _randn("token_embedding.weight", seed, (arch.vocab_size, tw), 0.02)
    sd["positional_embedding"] = _randn("positional_embedding", seed, (arch.context_length, tw), 0.01)
    affine("ln_final", tw)
    sd["text_projection"] = _randn("text_projection", seed, (tw, arch.embed_dim), tw ** -0.5, True)
    sd["logit_scale"] = torch.tensor(math.log(1 / 0.07), dtype=torch.float32)  # clip/model.py:291
    return sd
