"""TEST INFRASTRUCTURE — float64 restatement of CLIP's ModifiedResNet image tower and the error bounds of its kernels.

Written from the mathematics (clip/model.py:10-150 is the reference; nothing is copied): a three-conv stem (3x3 stride 2, 3x3,
3x3, each with BatchNorm in eval mode and ReLU, then a 2x2 average pool), four stages of bottleneck blocks (1x1 + BN + ReLU,
3x3 + BN + ReLU, 2x2 average pool where the block strides, 1x1 + BN; the identity through average pool + 1x1 + BN where the
shape changes; add, ReLU) and an attention pool (tokens [mean ; pixels] + positional embedding, multi-head attention with heads of
64 channels, only the mean token's output, an output projection).

``round16=True`` rounds to fp16 at exactly the points where the device tower (mvlpt_amd/csrc/conv.hip, resnet_fwd in engine.hip)
stores fp16: the image, every convolution output (which is the next convolution's input, the residual operand or the block output),
every pool output, the attention-pool tokens, q / k / v and the attention output.  BatchNorm's scale and shift are rounded to fp32
as the device holds them.  Everything else stays float64, so the result is the device's computation with exact accumulation: the
distance to the unrounded float64 result is what the number FORMATS cost, and what is left of the 1e-3 budget belongs to the
accumulation order.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24      # unit roundoff of fp32
U16 = 2.0 ** -11      # unit roundoff of fp16
SUB16 = 2.0 ** -25    # half the spacing of fp16 subnormals: the absolute floor of a rounding to fp16
CONV_KSTEP = 32       # the MFMA K-step the packed weight rows are padded to (conv.hip CV_BK)
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4")
SAMPLE = 64


def r16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16).to(torch.float64)


def _r(x, on):
    return r16(x) if on else x


def bn_affine(sd, prefix: str, fp32: bool):
    """BatchNorm with running statistics as scale = g / sqrt(var + 1e-5), shift = b - mean * scale."""
    g, b, m, v = (sd[f"{prefix}.{n}"].double() for n in ("weight", "bias", "running_mean", "running_var"))
    if fp32:      # the device forms both in fp32
        s = (g.float() / torch.sqrt(v.float() + 1e-5))
        return s.double(), (b.float() - m.float() * s).double()
    s = g / torch.sqrt(v + 1e-5)
    return s, b - m * s


def _conv_bn(sd, x, conv: str, bn: str, *, stride=1, relu=True, resid=None, round16=False):
    w = sd[conv + ".weight"].double()
    s, t = bn_affine(sd, bn, round16)
    y = F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    if resid is not None:
        y = y + resid
    if relu:
        y = y.clamp_min(0)
    return _r(y, round16)


def summarize(x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """mean, rms and a fixed 64-element sample (equally spaced in the flattened [B, C, H, W] map) of one stage output."""
    f = x.double().reshape(-1)
    idx = torch.arange(SAMPLE) * (f.numel() // SAMPLE)
    return {"mean": f.mean(), "rms": f.pow(2).mean().sqrt(), "sample": f[idx]}


def resnet_features(sd: Dict[str, torch.Tensor], image: torch.Tensor, layers, *, round16: bool = False,
                    stages: Optional[Dict[str, Dict[str, torch.Tensor]]] = None,
                    block_rms: Optional[List[float]] = None) -> torch.Tensor:
    """image [B, 3, R, R] -> features [B, output_dim], float64.  `stages` (a dict) receives summarize() of the stem and of every
    stage; `block_rms` (a list) the rms of every block output."""
    on = round16
    x = _r(image.double(), on)
    x = _conv_bn(sd, x, "visual.conv1", "visual.bn1", stride=2, round16=on)
    x = _conv_bn(sd, x, "visual.conv2", "visual.bn2", round16=on)
    x = _conv_bn(sd, x, "visual.conv3", "visual.bn3", round16=on)
    x = _r(F.avg_pool2d(x, 2), on)
    if stages is not None:
        stages["stem"] = summarize(x)
    for st, blocks in enumerate(layers):
        for i in range(blocks):
            q = f"visual.layer{st + 1}.{i}."
            stride = 2 if (i == 0 and st > 0) else 1
            y = _conv_bn(sd, x, q + "conv1", q + "bn1", round16=on)
            y = _conv_bn(sd, y, q + "conv2", q + "bn2", round16=on)
            if stride > 1:
                y = _r(F.avg_pool2d(y, stride), on)
            identity = x
            if q + "downsample.0.weight" in sd:
                if stride > 1:
                    identity = _r(F.avg_pool2d(x, stride), on)
                identity = _conv_bn(sd, identity, q + "downsample.0", q + "downsample.1", relu=False, round16=on)
            x = _conv_bn(sd, y, q + "conv3", q + "bn3", resid=identity, round16=on)
            if block_rms is not None:
                block_rms.append(float(x.pow(2).mean().sqrt()))
        if stages is not None:
            stages[f"layer{st + 1}"] = summarize(x)
    return attention_pool(sd, x, round16=on)


def attention_pool(sd, x: torch.Tensor, *, round16: bool = False) -> torch.Tensor:
    """x [B, E, H, W] -> [B, output_dim]: token 0 of multi-head attention over [mean ; pixels] + pos, heads of 64."""
    on = round16
    B, E, H, W = x.shape
    tok = x.reshape(B, E, H * W).permute(0, 2, 1)                                   # [B, HW, E]
    tok = torch.cat([tok.mean(dim=1, keepdim=True), tok], dim=1) + sd["visual.attnpool.positional_embedding"].double()
    tok = _r(tok, on)
    lin = lambda n, t: t @ sd[f"visual.attnpool.{n}_proj.weight"].double().T + sd[f"visual.attnpool.{n}_proj.bias"].double()
    q = _r(lin("q", tok[:, 0]), on)                                                # [B, E]
    k, v = _r(lin("k", tok), on), _r(lin("v", tok), on)                            # [B, T, E]
    o = single_query_attention(q, k, v)
    return lin("c", _r(o, on))


def single_query_attention(q, k, v) -> torch.Tensor:
    """q [B, E], k / v [B, T, E] -> [B, E]: per head of 64 channels softmax(q . k / 8) v."""
    B, T, E = k.shape
    h = E // 64
    s = torch.einsum("bhd,bthd->bht", q.reshape(B, h, 64), k.reshape(B, T, h, 64)) * 0.125
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bht,bthd->bhd", p, v.reshape(B, T, h, 64)).reshape(B, E)


# ------------------------------------------------------------------------------------------------ kernel-level references and bounds
# All bounds are first-order rounding analysis on float64 magnitudes (Higham, "Accuracy and Stability of Numerical Algorithms", §3.1:
# a sum of n terms accumulated in ANY order in a format of unit roundoff u is off by at most (n - 1) u sum|terms| / (1 - n u)); none
# of them is fitted to what the device returns.
def conv_kp(k: int, cin: int) -> int:
    return (k * k * cin + CONV_KSTEP - 1) // CONV_KSTEP * CONV_KSTEP


def conv_reference(x, w, scale, shift, *, stride=1, relu=False, resid=None, cin_pad=None):
    """NHWC x [B, H, W, Cin], w [Cout, Cin, k, k], scale / shift [Cout], resid NHWC -> (y NHWC float64, bound NHWC); cin_pad: the
    channel count the device pads Cin to (the 3-channel image travels as 8), which lengthens the accumulated K.

    Device arithmetic: fp32 accumulation of exact fp16 x fp16 products over the padded K (any order), then in fp32
    acc * scale + shift (one fma), + resid, ReLU, and ONE rounding to fp16.  With S = sum |x| |w|:
      |acc - exact| <= (Kp - 1) u32 S / (1 - Kp u32);  the fma, the residual add: one rounding each of a value bounded by
      S |scale| + |shift| + |resid|  ->  (Kp + 2) u32 (S |scale| + |shift| + |resid|) covers all three to first order (we take Kp + 4);
      the final rounding: u16 |y| + the subnormal floor.  ReLU is exact and 1-Lipschitz."""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    k = w.shape[-1]
    sc, sh = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    acc = F.conv2d(xd, wd, stride=stride, padding=k // 2)
    mag = F.conv2d(xd.abs(), wd.abs(), stride=stride, padding=k // 2) * sc.abs() + sh.abs()
    y = acc * sc + sh
    if resid is not None:
        rd = resid.double().permute(0, 3, 1, 2)
        y = y + rd
        mag = mag + rd.abs()
    if relu:
        y = y.clamp_min(0)
    kp = conv_kp(k, cin_pad or x.shape[-1])
    bound = (kp + 4) * U32 / (1 - (kp + 4) * U32) * mag + U16 * y.abs() + SUB16
    return y.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def avgpool_reference(x):
    """NHWC -> (y, bound): fp32 sum of four fp16 values (3 roundings of partial sums <= sum|x|), an exact * 0.25, one rounding."""
    xd = x.double().permute(0, 3, 1, 2)
    y = F.avg_pool2d(xd, 2)
    mag = F.avg_pool2d(xd.abs(), 2)
    bound = 3 * U32 * mag + U16 * y.abs() + SUB16
    return y.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def tokens_reference(x, pos):
    """x [B, HW, E] fp16, pos [1 + HW, E] fp32 -> (tok [B, 1 + HW, E], bound): the mean is an fp32 sum of HW terms, a division and
    an addition ((HW + 2) u32 of the magnitudes), the pixel rows one fp32 addition; one rounding to fp16 each."""
    xd, pd = x.double(), pos.double()
    HW = x.shape[1]
    tok = torch.cat([xd.mean(dim=1, keepdim=True), xd], dim=1) + pd
    mag = torch.cat([xd.abs().mean(dim=1, keepdim=True), xd.abs()], dim=1) + pd.abs()
    bound = (HW + 2) * U32 * mag + U16 * tok.abs() + SUB16
    return tok, bound


def query_reference(q, kv):
    """q [B, E], kv [B, T, 2E] = [K | V] (fp16 values) -> (out [B, E], bound [B, E]).

    Device arithmetic: s_t = (sum_64 q k) / 8 in fp32 (fma chain): |ds_t| <= 65 u32 sum|q||k| / 8.  e_t = exp(s_t - max) through
    exp2(x log2 e): the subtraction, the multiplication by log2 e and the hardware exp2 (1 ulp) give a relative error of at most
    (|s_t - max| + 3) u32 besides the propagated exp(2 max ds) - 1 <= 2.1 max ds.  Terms that far below the maximum that their
    weight is under 2^-40 are negligible, so |s_t - max| is capped at 28 in the bound.  With delta the bound on the relative error of every e_t, the
    normalised weights are off by at most 2 delta + T u32 relative (numerator, and the fp32 sum of T positive terms), and
    sum_t p_t v_t, an fp32 fma chain of T terms followed by a division, adds (T + 2) u32 sum p |v|.  One rounding to fp16."""
    B, T, E2 = kv.shape
    E = E2 // 2
    h = E // 64
    qd, kd, vd = q.double(), kv[..., :E].double(), kv[..., E:].double()
    out = single_query_attention(qd, kd, vd)
    qh, kh, vh = qd.reshape(B, h, 64), kd.reshape(B, T, h, 64), vd.reshape(B, T, h, 64)
    s = torch.einsum("bhd,bthd->bht", qh, kh) * 0.125
    ds = 65 * U32 * torch.einsum("bhd,bthd->bht", qh.abs(), kh.abs()) * 0.125
    delta = 2.1 * ds.amax(dim=-1, keepdim=True) + (28 + 3) * U32                   # [B, h, 1]
    p = torch.softmax(s, dim=-1)
    pv = torch.einsum("bht,bthd->bhd", p, vh.abs())                                # sum p |v|
    bound = ((2 * delta + T * U32) + (T + 2) * U32) * pv
    bound = bound.reshape(B, E) + U16 * out.abs() + SUB16
    return out, bound
