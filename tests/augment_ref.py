"""TEST INFRASTRUCTURE — numpy restatement of the pixel arithmetic behind the device augmentations
(`mvlpt_preprocess_aug`, csrc/preprocess.hip): Pillow's `convert("L")`, `ImageEnhance.Brightness / Color / Contrast`
(`Image.blend` against a degenerate image), `convert("HSV")`, HSV -> `convert("RGB")`, and what torchvision builds from
them on PIL images (ColorJitter, RandomGrayscale, pad + crop, Dassl's Cutout).  fp32 where Pillow's C uses `float`,
double where it uses `double`; numpy fuses no multiply-add.  tests/test_augment_ref.py holds every function to Pillow
itself; tests/test_hip_augment.py holds the kernels to these functions."""
from __future__ import annotations

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32, F64 = np.float32, np.float64


def luma(a: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] -> uint8 [...]: Pillow's ITU-R 601-2 L channel in 16-bit fixed point."""
    a = a.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d: np.ndarray, x: np.ndarray, alpha) -> np.ndarray:
    """Image.blend(degenerate d, image x, alpha) on 8-bit channels: d + alpha * (x - d) in fp32, truncated; clipped only when
    alpha extrapolates."""
    alpha = F32(alpha)
    d, x = d.astype(np.int32), x.astype(np.int32)
    t = d.astype(F32) + alpha * (x - d).astype(F32)
    if 0.0 <= alpha <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        mid = np.where((t > 0) & (t < 255), t, F32(0)).astype(np.int32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, mid)).astype(np.uint8)


def brightness(a: np.ndarray, f) -> np.ndarray:
    return blend(np.zeros_like(a), a, f)


def saturation(a: np.ndarray, f) -> np.ndarray:
    return blend(np.repeat(luma(a)[..., None], 3, -1), a, f)


def contrast_mean(a: np.ndarray) -> int:
    L = luma(a)
    return int(F64(int(L.astype(np.int64).sum())) / F64(L.size) + 0.5)


def contrast(a: np.ndarray, f) -> np.ndarray:
    return blend(np.full_like(a, contrast_mean(a)), a, f)


def grayscale(a: np.ndarray) -> np.ndarray:
    return np.repeat(luma(a)[..., None], 3, -1)


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb_to_hsv(a: np.ndarray) -> np.ndarray:
    r, g, b = (a[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(F32)
        s = cr / mx.astype(F32)
        rc, gc, bc = ((mx - c).astype(F32) / cr for c in (r, g, b))
        h = np.where(r == mx, bc - gc,
                     np.where(g == mx, (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32),
                              (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32)))
        h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
        h = np.where(flat, F32(0), h)
        s = np.where(flat, F32(0), s)
    H = _clip8((h.astype(F64) * 255.0).astype(np.int64))
    S = _clip8((s.astype(F64) * 255.0).astype(np.int64))
    return np.stack([H, S, mx.astype(np.uint8)], -1)


def _c_round(x):
    """C round() for x >= 0: halves away from zero (x - floor(x) is exact)."""
    fl = np.floor(x)
    return (fl + (x - fl >= 0.5)).astype(np.int64)


def hsv_to_rgb(a: np.ndarray) -> np.ndarray:
    H, S, V = a[..., 0], a[..., 1], a[..., 2]
    hh = H.astype(F32).astype(F64) * 6.0 / 255.0
    i = np.floor(hh)
    f = (hh - i).astype(F32)
    fs = (S.astype(F64) / 255.0).astype(F32)
    v = V.astype(F64)
    p = _clip8(_c_round(v * (1.0 - fs.astype(F64))))
    q = _clip8(_c_round(v * (1.0 - (fs * f).astype(F64))))
    t = _clip8(_c_round(v * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64)))))
    k = i.astype(np.int64) % 6
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    out = np.empty(a.shape, np.uint8)
    for c in range(3):
        out[..., c] = np.select([k == n for n in range(6)], [table[n][c] for n in range(6)])
    gray = S == 0
    for c in range(3):
        out[..., c] = np.where(gray, V, out[..., c])
    return out


def hue(a: np.ndarray, shift: int) -> np.ndarray:
    """torchvision adjust_hue on a PIL image: the HSV round trip runs even for a shift of 0 (and is not the identity)."""
    hsv = rgb_to_hsv(a)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def chain(a: np.ndarray, ops=(), factor=(1.0, 1.0, 1.0), hue_shift=0, gray=False, holes=()) -> np.ndarray:
    """The 8-bit image just before ToTensor: colour operations in the order of `ops`, grayscale, holes (top, left, h, w)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    for op in ops:
        if op == BRIGHTNESS:
            a = brightness(a, factor[0])
        elif op == CONTRAST:
            a = contrast(a, factor[1])
        elif op == SATURATION:
            a = saturation(a, factor[2])
        elif op == HUE:
            a = hue(a, hue_shift)
        else:
            raise ValueError(op)
    if gray:
        a = grayscale(a)
    a = a.copy()
    for (t, l, h, w) in holes:
        a[t:t + h, l:l + w] = 0
    return a


def window_with_fill(resized: np.ndarray, top: int, left: int, out_h: int, out_w: int) -> np.ndarray:
    """Window of `resized` that may hang over its sides; pixels outside are 0 (torchvision pad(fill=0) in front of a crop)."""
    rh, rw = resized.shape[:2]
    out = np.zeros((out_h, out_w, 3), np.uint8)
    y0, y1, x0, x1 = max(top, 0), min(top + out_h, rh), max(left, 0), min(left + out_w, rw)
    if y0 < y1 and x0 < x1:
        out[y0 - top:y1 - top, x0 - left:x1 - left] = resized[y0:y1, x0:x1]
    return out


def to_tensor_normalize(u8: np.ndarray, mean, std) -> np.ndarray:
    """[h, w, 3] uint8 -> [3, h, w] fp32 as torch's ToTensor + Normalize: two correctly rounded fp32 divisions."""
    x = u8.transpose(2, 0, 1).astype(F32) / F32(255)
    m, s = np.asarray(mean, F32)[:, None, None], np.asarray(std, F32)[:, None, None]
    return ((x - m) / s).astype(F32)


def golden_cases():
    """-> [(source, crop, resize, window, flip, fill, ops, factor, hue_shift, gray, holes, Pillow's bytes)], mean, std"""
    from tests.golden_util import load_npz
    g = load_npz("augment")
    cases = []
    for i in range(int(g["n"])):
        ct, cl, ch, cw, rh, rw, ot, ol, oh, ow, flip, fill = [int(v) for v in g[f"c{i}_desc"]]
        cases.append((g[f"c{i}_src"], (ct, cl, ch, cw), (rh, rw), (ot, ol, oh, ow), flip, fill, [int(v) for v in g[f"c{i}_ops"]],
                      g[f"c{i}_factor"], int(g[f"c{i}_misc"][0]), int(g[f"c{i}_misc"][1]),
                      [tuple(int(v) for v in r) for r in g[f"c{i}_holes"]], g[f"c{i}_u8"]))
    return cases, g["mean"], g["std"]


def reference_window(src, crop, resize, window, flip):
    """The flipped 8-bit window before any colour operation: the C oracle's resample, zero fill outside the resized image
    (the resample itself is pinned to Pillow by tests/test_preprocess_oracle.py)."""
    from oracle import preprocess_oracle as PO
    full = PO.resample_crop_u8(src, crop, resize, (0, 0, resize[0], resize[1]))
    win = window_with_fill(full, *window)
    return win[:, ::-1].copy() if flip else win
