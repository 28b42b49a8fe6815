"""Device JPEG decode against the host route, on one GPU (the figures of DESIGN.md row f3c).

    python tools/jpeg_bench.py [--batch 256] [--runs 7] [--threads 16] [--size 224] [--out FILE.json]
    python tools/jpeg_bench.py --decode-only 20 [--restart]      # decodes alone, for `rocprofv3 --kernel-trace --stats -- python ...`

Input: synthetic photo-like images (a smooth random field plus noise), 375 x 500, quality 90, 4:2:0, written once without and once
with a restart interval of one MCU row.  Routes, each timed from host bytes to the normalised [B, 3, size, size] batch, host clock
around work that ends in a device synchronise, median of `--runs` runs taken alternately:
  host     Pillow decode in a `--threads` pool -> DeviceTransform.__call__ (pack, upload of the pixels, mvlpt_preprocess)
  device   DeviceTransform.from_encoded: pack and upload of the file bytes, mvlpt_jpeg_decode, mvlpt_preprocess; check=False
and the device decode alone (mvlpt_jpeg_decode on bytes already on the device).  One JSON line per (batch, restart) on stdout."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic(n, seed=0, H=375, W=500):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        low = rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)
        a = np.asarray(Image.fromarray(low).resize((W, H), Image.BICUBIC)).astype(np.int16)
        a = a + rng.normal(0, 12, (H, W, 1)).astype(np.int16) + rng.integers(-6, 7, (H, W, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def encode(images, restart):
    from PIL import Image
    blobs = []
    for a in images:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=90, subsampling=2, **(dict(restart_marker_rows=1) if restart else {}))
        blobs.append(buf.getvalue())
    return blobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--decode-only", type=int, default=0)
    ap.add_argument("--restart", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from mvlpt_amd import jpeg
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.transforms import DeviceTransform
    from mvlpt_amd.weights import ARCHS
    assert torch.cuda.is_available(), "jpeg_bench needs a GPU"
    eng = Engine(ARCHS["tiny"], "fp16")
    base = synthetic(256)
    sets = {r: encode(base, r) for r in ((args.restart,) if args.decode_only else (False, True))}

    def sync():
        torch.cuda.synchronize()

    if args.decode_only:
        blobs = sets[args.restart]
        for _ in range(args.decode_only):
            jpeg.decode_batch(eng, blobs, check=False)
        sync()
        print(json.dumps({"decode_only": args.decode_only, "batch": len(blobs), "restart": args.restart}))
        return

    pool = ThreadPoolExecutor(args.threads)
    lines = []
    for B in args.batch:
        for restart, blobs256 in sets.items():
            blobs = (blobs256 * ((B + 255) // 256))[:B]
            tr = DeviceTransform(eng, size=args.size, train=False)
            infos = [jpeg.probe(b) for b in blobs]

            def host_route():
                arrays = list(pool.map(jpeg.pillow_rgb, blobs))
                return tr(arrays)

            def device_route():
                return tr.from_encoded(blobs, check=False)

            def pillow_only():
                return list(pool.map(jpeg.pillow_rgb, blobs))

            def decode_only():
                return jpeg.decode_batch(eng, blobs, check=False, infos=infos)

            want, got = host_route(), device_route()
            sync()
            assert torch.equal(want, got), "the two routes differ"
            st = decode_only()[3]
            assert not st.cpu().numpy().any()
            routes = {"host": host_route, "device": device_route, "pillow_pool": pillow_only, "device_decode_from_host_bytes": decode_only}
            times = {k: [] for k in routes}
            for _ in range(args.runs):
                for k, fn in routes.items():                         # alternately
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    times[k].append(time.perf_counter() - t0)
            med = {k: statistics.median(v) for k, v in times.items()}
            pixels = sum(f.height * f.width * 3 for f in infos)
            line = {"batch": B, "restart_rows": restart, "runs": args.runs, "threads": args.threads,
                    "file_bytes": sum(len(b) for b in blobs), "pixel_bytes": pixels, "workspace_bytes": jpeg.workspace_bytes(infos),
                    "images_per_s": {k: round(B / v, 1) for k, v in med.items()},
                    "ms_median": {k: round(v * 1e3, 3) for k, v in med.items()},
                    "ms_min_max": {k: [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)] for k, v in times.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
