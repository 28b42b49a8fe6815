"""Writes tests/golden/augment.npz: whole augmentation chains computed by Pillow alone -- `crop`, `resize(BICUBIC)`,
`ImageOps.expand(fill=0)` + `crop` (torchvision's pad in front of RandomCrop), `transpose`, `ImageEnhance.Brightness / Contrast /
Color`, the HSV round trip of torchvision's adjust_hue (`convert("HSV")`, H += shift, `convert("RGB")`), `convert("L")` -- and
Cutout's zeroed rectangles.  Data only: sources, parameters and Pillow's bytes.  The fp32 side (ToTensor / Normalize) is two torch
divisions the tests do themselves.
Usage: python tools/make_augment_golden.py"""
import os

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "augment.npz")
B, C, S, H = 0, 1, 2, 3

# (source H, W, content, crop (top, left, h, w), resized (rh, rw), window (top, left, h, w), flip,
#  [(operation, factor or hue shift)], grayscale, holes [(top, left, h, w)])
SPECS = [
    (40, 50, "noise", (0, 0, 40, 50), (32, 32), (0, 0, 32, 32), 0, [(B, 1.3), (C, 0.7), (S, 1.5), (H, 20)], 0, []),
    (32, 32, "noise", (0, 0, 32, 32), (32, 32), (0, 0, 32, 32), 0, [(H, 0)], 0, []),                    # the round trip alone
    (48, 36, "smooth", (3, 2, 40, 30), (32, 32), (0, 0, 32, 32), 1, [(C, 0.0)], 1, []),
    (30, 30, "noise", (0, 0, 30, 30), (32, 32), (-4, -3, 32, 32), 1, [(S, 0.0), (B, 1.0)], 0, [(5, 20, 16, 12)]),   # over top and left
    (20, 25, "smooth", (0, 0, 20, 25), (24, 24), (-4, -4, 32, 32), 0, [(C, 1.8), (H, 128)], 0, []),       # over all four sides
    (50, 50, "noise", (1, 1, 48, 49), (48, 48), (0, 0, 48, 48), 0, [(H, 255), (S, 2.0), (C, 0.5), (B, 0.5)], 0,
     [(0, 0, 10, 10), (5, 5, 16, 16)]),
    (40, 60, "smooth", (0, 0, 40, 60), (33, 47), (0, 0, 33, 47), 1, [], 1, []),
    (5, 5, "noise", (0, 0, 5, 5), (1, 1), (0, 0, 1, 1), 0, [(C, 1.5), (B, 2.0)], 0, []),
    (32, 32, "binary", (0, 0, 32, 32), (32, 32), (40, 0, 32, 32), 0, [(B, 1.5), (C, 0.5)], 0, []),       # wholly outside
    (45, 45, "noise", (0, 0, 45, 45), (32, 32), (0, 0, 32, 32), 1, [(S, 0.3), (H, 1), (C, 1.2)], 1,
     [(0, 0, 4, 4), (28, 28, 4, 4), (10, 0, 8, 32), (12, 4, 3, 3)]),
    (36, 36, "noise", (0, 0, 36, 36), (32, 32), (3, -2, 32, 32), 0, [], 0, []),                          # over bottom and left
    (32, 40, "smooth", (0, 0, 32, 40), (32, 32), (0, 5, 32, 32), 1, [(B, 0.0)], 0, []),                  # vertical pass skipped, over right
    (44, 28, "binary", (2, 0, 40, 28), (48, 48), (0, 0, 48, 48), 0, [(B, 0.25), (H, 77), (S, 1.0), (C, 1.0)], 0, [(40, 40, 8, 8)]),
]


def hue(img, shift):
    h, s, v = img.convert("HSV").split()
    nh = ((np.asarray(h).astype(np.int32) + shift) & 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")


def main():
    rng = np.random.default_rng(11)
    out = {"mean": np.array([0.48145466, 0.4578275, 0.40821073], np.float32), "std": np.array([0.26862954, 0.26130258, 0.27577711], np.float32)}
    for i, (Hs, Ws, kind, (ct, cl, ch, cw), (rh, rw), (ot, ol, oh, ow), flip, ops, gray, holes) in enumerate(SPECS):
        if kind == "noise":
            a = rng.integers(0, 256, (Hs, Ws, 3))
        elif kind == "binary":
            a = rng.integers(0, 2, (Hs, Ws, 3)) * 255
        else:
            yy, xx = np.mgrid[0:Hs, 0:Ws]
            a = np.stack([127 + 120 * np.sin(yy / 7.0 + xx / 11.0), (xx * 255) // max(Ws - 1, 1),
                          127 + 100 * np.cos(yy / 3.0) * np.sin(xx / 5.0)], -1) + rng.integers(-6, 7, (Hs, Ws, 3))
        a = np.clip(a, 0, 255).astype(np.uint8)
        img = Image.fromarray(a).crop((cl, ct, cl + cw, ct + ch)).resize((rw, rh), Image.BICUBIC)
        fill = int(ot < 0 or ol < 0 or ot + oh > rh or ol + ow > rw)
        pad = max(0, -ot, -ol, ot + oh - rh, ol + ow - rw)
        img = ImageOps.expand(img, border=pad, fill=0).crop((ol + pad, ot + pad, ol + pad + ow, ot + pad + oh))
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        factor, shift = np.ones(3, np.float32), 0
        for op, v in ops:
            if op == H:
                shift = int(v)
                img = hue(img, shift)
            else:
                factor[op] = v
                enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op]
                img = enh(img).enhance(float(factor[op]))             # Pillow's C takes the factor as a float
        if gray:
            img = Image.merge("RGB", (img.convert("L"),) * 3)
        u8 = np.asarray(img).copy()
        for (t, l, h, w) in holes:
            u8[t:t + h, l:l + w] = 0
        out[f"c{i}_src"] = a
        out[f"c{i}_desc"] = np.array([ct, cl, ch, cw, rh, rw, ot, ol, oh, ow, flip, fill], np.int64)
        out[f"c{i}_ops"] = np.array([op for op, _ in ops], np.int64)
        out[f"c{i}_factor"] = factor
        out[f"c{i}_misc"] = np.array([shift, gray], np.int64)
        out[f"c{i}_holes"] = np.array(holes, np.int64).reshape(-1, 4)
        out[f"c{i}_u8"] = u8
    out["n"] = np.int64(len(SPECS))
    np.savez_compressed(OUT, **out)
    print("[golden] augment:", len(SPECS), "cases,", os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
