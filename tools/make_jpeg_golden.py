"""Writes tests/golden/jpeg.npz with Pillow alone: JPEG files and the RGB pixels `Image.open(...).convert("RGB")` gives for them.

    python tools/make_jpeg_golden.py            # rewrites the fixture

Arrays per case k: jpeg_k (uint8 bytes), rgb_k (uint8 [H, W, 3]; absent when Pillow cannot read the file), and the lists `names`
and `kinds` (0 the device decodes it, 1 fallback route, 2 malformed entropy data).  Cases:
  - 7 sizes from 1 x 1 to 37 x 45 x {smooth gradient, uniform noise} x {4:4:4, 4:2:2, 4:2:0, grayscale} x {quality 90; quality 30 with
    optimised Huffman tables; quality 75 with a restart interval of 1 MCU}: 168 files;
  - quality 100, and a restart interval of one MCU row, on two of the sizes, noise, every sampling;
  - 100 x 75 (segments that span MCU rows), every sampling: gradient at quality 90, noise at quality 75 with a restart interval of 5 MCUs
    and of one MCU row;
  - fallback: progressive, CMYK, 4:4:0 (a 4:2:2 file with the luma factors and the image sides swapped in its frame header: the same
    MCU count and block order, so a valid file that libjpeg reads);
  - malformed: a file cut in the middle of its scan, and one with a single entropy byte replaced, the first candidate from the middle
    of the scan that tests/jpeg_ref.py flags (status > 0) and Pillow still reads."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref  # noqa: E402

SIZES = [(1, 1), (8, 8), (17, 23), (33, 16), (16, 33), (9, 50), (37, 45)]          # (width, height)
SAMPLINGS = [("444", 0), ("422", 1), ("420", 2), ("gray", None)]
SETTINGS = [("q90", dict(quality=90)), ("q30opt", dict(quality=30, optimize=True)), ("q75rst1", dict(quality=75, restart_marker_blocks=1))]


def content(kind, W, H, rng):
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx + yy) * 255 // max(W + H - 2, 1)], 2).astype(np.uint8)


def encode(a, sampling, **kw):
    buf = io.BytesIO()
    if sampling is None:
        Image.fromarray(a).convert("L").save(buf, "JPEG", **kw)
    else:
        Image.fromarray(a).save(buf, "JPEG", subsampling=sampling, **kw)
    return buf.getvalue()


def pillow_rgb(blob):
    try:
        return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
    except Exception:
        return None


def main():
    rng = np.random.default_rng(20240)
    cases = []                                                   # (name, kind, blob)
    for W, H in SIZES:
        for kind in ("smooth", "noise"):
            a = content(kind, W, H, rng)
            for sname, s in SAMPLINGS:
                for ename, kw in SETTINGS:
                    cases.append((f"{W}x{H}_{kind}_{sname}_{ename}", 0, encode(a, s, **kw)))
    for W, H in ((17, 23), (37, 45)):
        a = content("noise", W, H, rng)
        for sname, s in SAMPLINGS:
            cases.append((f"{W}x{H}_noise_{sname}_q100", 0, encode(a, s, quality=100)))
            cases.append((f"{W}x{H}_noise_{sname}_q75rstrow", 0, encode(a, s, quality=75, restart_marker_rows=1)))
    W, H = 100, 75
    for sname, s in SAMPLINGS:
        cases.append((f"{W}x{H}_smooth_{sname}_q90", 0, encode(content("smooth", W, H, rng), s, quality=90)))
        a = content("noise", W, H, rng)
        cases.append((f"{W}x{H}_noise_{sname}_q75rst5", 0, encode(a, s, quality=75, restart_marker_blocks=5)))
        cases.append((f"{W}x{H}_noise_{sname}_q75rstrow", 0, encode(a, s, quality=75, restart_marker_rows=1)))
    a = content("noise", 37, 45, rng)
    cases.append(("fallback_progressive", 1, encode(a, 2, quality=90, progressive=True)))
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (45, 37, 4)).astype(np.uint8), "CMYK").save(buf, "JPEG", quality=90)
    cases.append(("fallback_cmyk", 1, buf.getvalue()))
    blob = bytearray(encode(a, 1, quality=90))
    k = blob.index(b"\xff\xc0")
    assert blob[k + 11] == 0x21                                  # SOF0: FF C0, length, precision, height, width, Nf, id, factors
    blob[k + 5:k + 9] = blob[k + 7:k + 9] + blob[k + 5:k + 7]    # height <-> width
    blob[k + 11] = 0x12
    cases.append(("fallback_440", 1, bytes(blob)))
    good = encode(a, 2, quality=90)
    P = jpeg_ref.parse(good)
    b, e = P.segs[0]
    cases.append(("malformed_cut", 2, good[:(b + e) // 2]))
    for pos in range((b + e) // 2, e):
        for v in (0x00, 0x55, 0xAA, 0xF7):
            m = good[:pos] + bytes([v]) + good[pos + 1:]
            if v == good[pos] or good[pos] == 0xFF or good[pos - 1] == 0xFF:
                continue
            Q = jpeg_ref.parse(m)
            if Q.route == 0 and jpeg_ref.decode(m)[1] > 0 and pillow_rgb(m) is not None:
                cases.append(("malformed_byte", 2, m))
                break
        else:
            continue
        break
    assert cases[-1][0] == "malformed_byte"
    out = {"names": np.array([c[0] for c in cases]), "kinds": np.array([c[1] for c in cases], np.int32)}
    for k, (name, kind, blob) in enumerate(cases):
        out[f"jpeg_{k}"] = np.frombuffer(blob, np.uint8)
        rgb = pillow_rgb(blob)
        if rgb is not None:
            out[f"rgb_{k}"] = rgb
    path = os.path.join(ROOT, "tests", "golden", "jpeg.npz")
    np.savez_compressed(path, **out)
    print(f"{len(cases)} cases, Pillow {Image.__version__}, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
