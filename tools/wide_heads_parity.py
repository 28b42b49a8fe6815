"""Full-size feature parity of the image tower against the CPU oracle (fp32), as a fraction of max|ref|. GPU box only.

  python tools/wide_heads_parity.py [ARCH ...]      (default: ViT-H/14 ViT-L/14)

Random weights of the named architectures (mvlpt_amd.weights.make_state_dict, seed 2), 2 images, activation quick_gelu and gelu.  The
reference cannot build a ViT-H/14 (clip/model.py:268: heads = width // 64), so the oracle (oracle/clip_oracle.py, heads = 16) is the
truth here; ViT-L/14 runs beside it as the figure of a tower the reference does pin."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mvlpt_amd.model import FrozenCLIP
from mvlpt_amd.weights import get_arch, make_state_dict
from oracle import clip_oracle as O

for name in sys.argv[1:] or ["ViT-H/14", "ViT-L/14"]:
    arch = get_arch(name)
    sd = make_state_dict(arch, 2)
    image = torch.randn(2, 3, arch.image_resolution, arch.image_resolution, generator=torch.Generator().manual_seed(5))
    clip = FrozenCLIP(sd, compute_dtype="fp16", arch=arch)
    for act in ("quick_gelu", "gelu"):
        clip.engine.set_activation(act)
        got = clip.encode_image(image).double().cpu()
        quick = O.quick_gelu
        if act == "gelu":
            O.quick_gelu = lambda u: torch.nn.functional.gelu(u)
        try:
            with torch.no_grad():
                want, _ = O.image_encoder_fwd(sd, image, None, None, heads=arch.vision_heads, need_bwd=False)
        finally:
            O.quick_gelu = quick
        err = float((got - want.double()).abs().max()) / float(want.abs().max())
        print(f"{name} ({arch.vision_heads} heads of {arch.vision_head_width}, {arch.grid ** 2 + 1} tokens) {act}: "
              f"features max|err| / max|ref| = {err:.2e}", flush=True)
    del clip
