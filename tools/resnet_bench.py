"""The ResNet image towers (RN50, RN101): `FrozenCLIP.encode_image` on the HIP engine next to the same tower written with stock
torch-ROCm ops on the same GPU, and a per-layer table of the implicit-GEMM convolution kernel.

    python tools/resnet_bench.py [--archs RN50 RN101] [--batch 256] [--rounds 7] [--layer-reps 5]

Tower: the two routes alternate inside one process (`--rounds` times after a warm-up of each); a time is a device-event interval
around one whole forward, reported as median and minimum and as images/s.  The stock route is fp16, channels-last, `F.conv2d` with
BatchNorm applied as the same per-channel scale / shift, `F.avg_pool2d`, and the attention pool as `F.linear` + softmax; its features
are compared with the engine's on the same images before anything is timed (a faster route that computes something else is not
faster).  Layers: every distinct convolution of the tower (input size, channels, kernel, stride, residual) is timed alone through
`mvlpt_op_conv2d` at the same batch — median of `--layer-reps` device-event intervals — and listed with its count in the tower, its
share of the summed convolution time and its TFLOP/s on 2 M N K (the K of the arithmetic, not the padded one).
Prints the table and one JSON line per architecture.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


class TorchTower:
    """The tower on stock ops: fp16, channels-last, BatchNorm as scale / shift."""

    def __init__(self, sd, arch, device):
        self.arch = arch
        h = lambda v: v.to(device).half()
        self.sd = {}
        for k, v in sd.items():
            if not k.startswith("visual.") or k.endswith("num_batches_tracked"):
                continue
            self.sd[k] = h(v).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to(device).float()
        self.bn = {}
        for k in list(self.sd):
            if k.endswith(".running_var"):
                p = k[:-len(".running_var")]
                s = self.sd[p + ".weight"] / torch.sqrt(self.sd[k] + 1e-5)
                self.bn[p] = (s.half().view(1, -1, 1, 1), (self.sd[p + ".bias"] - self.sd[p + ".running_mean"] * s).half().view(1, -1, 1, 1))

    def conv(self, x, conv, bn, stride=1, relu=True, resid=None):
        w = self.sd[conv + ".weight"]
        s, t = self.bn[bn]
        y = F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2) * s + t
        if resid is not None:
            y = y + resid
        return F.relu(y) if relu else y

    @torch.no_grad()
    def __call__(self, image):
        x = image.half().contiguous(memory_format=torch.channels_last)
        x = self.conv(x, "visual.conv1", "visual.bn1", stride=2)
        x = self.conv(x, "visual.conv2", "visual.bn2")
        x = self.conv(x, "visual.conv3", "visual.bn3")
        x = F.avg_pool2d(x, 2)
        for st, blocks in enumerate(self.arch.vision_layers):
            for i in range(blocks):
                q = f"visual.layer{st + 1}.{i}."
                stride = 2 if (i == 0 and st > 0) else 1
                y = self.conv(x, q + "conv1", q + "bn1")
                y = self.conv(y, q + "conv2", q + "bn2")
                if stride > 1:
                    y = F.avg_pool2d(y, stride)
                identity = x
                if q + "downsample.0.weight" in self.sd:
                    if stride > 1:
                        identity = F.avg_pool2d(x, stride)
                    identity = self.conv(identity, q + "downsample.0", q + "downsample.1", relu=False)
                x = self.conv(y, q + "conv3", q + "bn3", resid=identity)
        B, E, H, W = x.shape
        tok = x.flatten(2).permute(0, 2, 1)
        tok = torch.cat([tok.float().mean(dim=1, keepdim=True).half(), tok], dim=1) + self.sd["visual.attnpool.positional_embedding"].half()
        lin = lambda n, v: F.linear(v, self.sd[f"visual.attnpool.{n}_proj.weight"].half(), self.sd[f"visual.attnpool.{n}_proj.bias"].half())
        q, k, v = lin("q", tok[:, 0]), lin("k", tok), lin("v", tok)
        h = E // 64
        s = torch.einsum("bhd,bthd->bht", q.view(B, h, 64).float(), k.view(B, -1, h, 64).float()) * 0.125
        o = torch.einsum("bht,bthd->bhd", torch.softmax(s, -1), v.view(B, -1, h, 64).float()).reshape(B, E)
        return lin("c", o.half()).float()


def conv_layers(arch):
    """(name, H in, Cin, Cout, k, stride, residual) of every convolution, in tower order."""
    w, R = arch.vision_width, arch.image_resolution
    out = [("stem.conv1", R, 8, w // 2, 3, 2, False), ("stem.conv2", R // 2, w // 2, w // 2, 3, 1, False),
           ("stem.conv3", R // 2, w // 2, w, 3, 1, False)]
    H, inplanes = R // 4, w
    for st, blocks in enumerate(arch.vision_layers):
        planes = w << st
        for i in range(blocks):
            stride = 2 if (i == 0 and st > 0) else 1
            q = f"layer{st + 1}.{i}."
            out.append((q + "conv1", H, inplanes, planes, 1, 1, False))
            out.append((q + "conv2", H, planes, planes, 3, 1, False))
            if stride > 1 or inplanes != planes * 4:
                out.append((q + "downsample", H // stride, inplanes, planes * 4, 1, 1, False))
            out.append((q + "conv3", H // stride, planes, planes * 4, 1, 1, True))
            inplanes, H = planes * 4, H // stride
    return out


def layer_table(arch, B, reps):
    from mvlpt_amd import engine as E
    groups = {}
    for name, H, cin, cout, k, stride, resid in conv_layers(arch):
        groups.setdefault((H, cin, cout, k, stride, resid), []).append(name)
    rows = []
    for (H, cin, cout, k, stride, resid), names in groups.items():
        x = torch.randn(B, H, H, cin, device="cuda").half()
        wp = E.op_pack_conv_weight(torch.randn(cout, cin, k, k, device="cuda") * (2.0 / (cin * k * k)) ** 0.5, cin)
        scale, shift = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        ho = E.conv_out_size(H, k, stride)
        out = torch.empty(B, ho, ho, cout, device="cuda", dtype=torch.float16)
        r = torch.randn(B, ho, ho, cout, device="cuda").half() if resid else None
        run = lambda: E.op_conv2d(x, wp, scale, shift, k, stride, True, r, out=out)
        run()
        ms = statistics.median(timed(run)[0] for _ in range(reps))
        flops = 2.0 * B * ho * ho * cout * k * k * cin
        rows.append({"first": names[0], "count": len(names), "H": H, "Cin": cin, "Cout": cout, "k": k, "stride": stride, "resid": resid,
                     "ms": ms, "tflops": flops / ms * 1e-9, "total_ms": ms * len(names), "total_flops": flops * len(names)})
        del x, out, r
    total = sum(r["total_ms"] for r in rows)
    print(f"{'layer (first of its shape)':28s} {'n':>3s} {'H':>4s} {'Cin':>5s} {'Cout':>5s} k s r {'ms':>8s} {'TF':>7s} {'n x ms':>8s} {'share':>6s}")
    for r in rows:
        print(f"{r['first']:28s} {r['count']:3d} {r['H']:4d} {r['Cin']:5d} {r['Cout']:5d} {r['k']} {r['stride']} {int(r['resid'])} "
              f"{r['ms']:8.3f} {r['tflops']:7.1f} {r['total_ms']:8.3f} {100 * r['total_ms'] / total:5.1f}%")
    tf = sum(r["total_flops"] for r in rows) / total * 1e-9
    print(f"{'all convolutions':28s} {sum(r['count'] for r in rows):3d} {'':27s} {total:8.3f} ms, {tf:.1f} TF on 2 M N K")
    return rows, total, tf


def main(argv=None) -> int:
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import RESNET_ARCHS, make_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--archs", nargs="+", default=["RN50", "RN101"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--layer-reps", type=int, default=5)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "resnet_bench needs a GPU"
    for name in args.archs:
        arch = RESNET_ARCHS[name]
        sd = make_state_dict(arch, 0)
        clip = FrozenCLIP(sd, compute_dtype="fp16", device="cuda:0")
        stock = TorchTower(sd, arch, "cuda:0")
        B = args.batch
        image = torch.randn(B, 3, arch.image_resolution, arch.image_resolution, generator=torch.Generator().manual_seed(1)).cuda()
        ours, theirs = clip.encode_image(image), stock(image)          # warm-up of both, and the comparison
        torch.cuda.synchronize()
        diff = float((ours - theirs).abs().max()) / float(ours.abs().max())
        clip.encode_image(image), stock(image)
        t_hip, t_stock = [], []
        for _ in range(args.rounds):
            t_hip.append(timed(lambda: clip.encode_image(image))[0])
            t_stock.append(timed(lambda: stock(image))[0])
        print(f"== {name}, batch {B}")
        rows, conv_ms, conv_tf = layer_table(arch, B, args.layer_reps)
        res = {"arch": name, "batch": B, "rounds": args.rounds,
               "hip_ms_median": statistics.median(t_hip), "hip_ms_min": min(t_hip),
               "stock_ms_median": statistics.median(t_stock), "stock_ms_min": min(t_stock),
               "hip_images_per_s": 1000.0 * B / statistics.median(t_hip), "stock_images_per_s": 1000.0 * B / statistics.median(t_stock),
               "features_hip_vs_stock_rel_max": diff, "conv_ms_sum_of_layers": conv_ms, "conv_tflops": conv_tf,
               "layers": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items() if k != "total_flops"} for r in rows]}
        print(json.dumps(res))
        del clip, stock, image
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
