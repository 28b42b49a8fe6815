"""Float64 references, seeded inputs, per-element error bounds and bit-exact format statements of the LayerNorm kernels
(mvlpt_amd/csrc/norm.hip), the operand-format kernels and the patch extraction (mvlpt_amd/csrc/glue.hip).  Plain torch on whatever
device the tensors live on; nothing here launches a kernel of the library.  tests/test_norm_format_ref.py checks the module without a
GPU; tests/test_hip_norm_matrix.py and tests/test_hip_formats.py use it.

LayerNorm reference.  On the fp32 inputs the kernel reads, in float64: mean, BIASED variance, rstd = (var + 1e-5)^-1/2,
xhat = (x - mean) rstd, y = xhat gamma + beta; backward (oracle/clip_oracle.py layernorm_bwd): gg = dy gamma, s1 = mean(gg),
s2 = mean(gg xhat), dx = rstd (gg - s1 - xhat s2), out = dx + resid.  Row r of the call is row r * row_mul of x / resid / out; dy and the
forward's y are dense.

Per-element bound (derived; it holds for any summation order; never fitted to device output).  u = 2^-24, every fp32 operation rounds
once, a sum of d terms loses at most (d - 1) u of the sum of its magnitudes; each quantity's error from the float64 magnitudes of the
ones before it, first order in u for the roundings themselves, but a product of two quantities that both carry a propagated error keeps
the product of the two errors, (|a| + e_a)(|b| + e_b) - |a b|: on a constant row c, xhat and s2 are exactly 0 and those products are all
the error there is (the fp32 mean of 1028 equal values is off by up to d u |x|, and rstd = eps^-1/2 = 316 multiplies that):
    e_mean = d u mean|x|                                    (the sum and the division)
    e_c    = e_mean + u |c|                                 c = x - mean
    e_var  = mean((2 |c| + e_c) e_c) + (d + 3) u (var + eps)  (the squares, their sum, the division, + eps)
    e_rstd = rstd (e_var / (2 (var + eps)) + E_RSQ)
    e_xhat = rstd e_c + (|c| + e_c) e_rstd + u |xhat|
    e_y    = |gamma| e_xhat + u |xhat gamma| + u |y|
    e_gg   = u |gg|
    e_s1   = mean(e_gg) + d u mean|gg|
    e_t    = |xhat| e_gg + (|gg| + e_gg) e_xhat + u |t|     t = gg xhat
    e_s2   = mean(e_t) + d u mean|t|
    e_p    = |s2| e_xhat + (|xhat| + e_xhat) e_s2 + u |p|   p = xhat s2
    e_in   = e_gg + e_s1 + e_p + 2 u (|gg| + |s1| + |p|)    (two subtractions in either order)
    e_dx   = |inner| e_rstd + (rstd + e_rstd) e_in + u |dx|
    e_out  = e_dx + u (|dx| + |resid|)                      (the residual add)
and the stored value is rounded once more to the output format, exactly as tests/gemm_ref.py does it:
    |got - ref| <= u_out (|ref| + e) + floor + e
with u_out and the subnormal floors of gemm_ref (U_OUT16, U_PAIR, U_MIXED; 2^-24 for fp32).
E_RSQ is the one term that is NOT derivable here: the relative error of the device's rsqrtf.  Like gemm_ref's E_FN it is 4x the largest
relative error of a plain fp32 host torch.rsqrt against float64 on the tests' own var + eps values.  Measured over every width and row
kind of the GPU matrix (DESIGN.md "LayerNorm and format kernel tests"): 8.60e-8 -> E_RSQ below; tests/test_norm_format_ref.py
re-measures it and holds the constant to 4x.

Formats (bit-exact statements; inputs stay below 65504 in magnitude after the scale: a value whose hi half rounds to infinity is outside
the formats, common.h "every finite fp16 value"):
    plain  round16(fl32(x s))                       pair   hi = round16(v), lo = round16(v - hi) (the subtraction is exact in fp32)
    mixed  gemm_ref.encode_mixed (hi as above, byte = e5m2((v - hi) 2^LO8_EXP), bf16 clamped to +-57344)
    pack_weight  round16(w) at a pitch, zero tail   pack_weight_t  its transpose (the tail is not written)
    cast_to_f32  exact widening
    patchify  out[b G^2 + gy G + gx][c P^2 + ky P + kx] = round16(image[b][c][gy P + ky][gx P + kx]), zero from column 3 P^2 on
"""
import functools

import torch

from tests.gemm_ref import LO8_EXP, U_MIXED, U_OUT16, U_PAIR, decode_lo8, encode_mixed, violations  # noqa: F401

LN_EPS = 1e-5
U32 = 2.0 ** -24
E_RSQ = 3.45e-7          # 4x the measured fp32 host error of rsqrt (module docstring)
DTYPES = [torch.float16, torch.bfloat16]
IDS = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}

# the GPU matrix (tests/test_hip_norm_matrix.py); the CPU test walks the same widths
DIRECT_ROWS = [1, 3, 4, 5, 203]
DIRECT_D = [4, 128, 252, 256, 260, 768, 1028, 2048]
STREAM_ROWS = [4096, 4097, 5123]
STREAM_D = {260: 2, 768: 3, 1024: 4, 1280: 8, 2048: 8}           # d -> NV of the grid-stride instantiation
ALL_D = sorted(set(DIRECT_D) | set(STREAM_D))
ROW_KINDS = ["gaussian", "large_mean", "constant", "outlier", "tiny", "zero"]


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=4)
def ln_inputs(rows, d):
    """Seeded fp32 operands of a LayerNorm over `rows` rows: row r of x is of kind ROW_KINDS[r % 6], so every tensor mixes rows whose
    statistics differ by orders of magnitude and no tensor-level scale can hide one.  -> dict(x, gamma, beta, dy, resid)."""
    g = torch.Generator().manual_seed(7919 * d + rows)
    x = torch.randn(rows, d, generator=g)
    kind = torch.arange(rows) % len(ROW_KINDS)
    out = x * 3 + 0.5                                                   # gaussian
    out = torch.where((kind == 1).view(-1, 1), 1000 + 1e-2 * x, out)    # large mean, small spread
    const = torch.randn(rows, 1, generator=g) * 2
    out = torch.where((kind == 2).view(-1, 1), const.expand(rows, d), out)      # variance 0: rstd = eps^-1/2
    spike = x.clone()
    spike[torch.arange(rows), torch.randint(0, d, (rows,), generator=g)] = 300.0
    out = torch.where((kind == 3).view(-1, 1), spike, out)              # one outlier channel among unit values
    out = torch.where((kind == 4).view(-1, 1), 1e-4 * x, out)           # tiny: eps matters
    out = torch.where((kind == 5).view(-1, 1), torch.zeros(()), out)    # all zero
    return dict(x=out.contiguous(), gamma=1.0 + 0.3 * torch.randn(d, generator=g), beta=0.2 * torch.randn(d, generator=g),
                dy=torch.randn(rows, d, generator=g), resid=torch.randn(rows, d, generator=g))


def row_kind(rows):
    return torch.arange(rows) % len(ROW_KINDS)


# ------------------------------------------------------------------------------------------------ float64 reference and bound
def out_rounding(dtype, fmt):
    """(relative rounding, absolute floor) of a stored value; fmt: 0 plain, 1 hi|lo pair, 2 mixed pair."""
    if dtype == torch.float32:
        return U32, 0.0
    f16 = dtype == torch.float16
    if fmt == 0:
        return U_OUT16[dtype], (2.0 ** -25 if f16 else 0.0)
    if fmt == 1:
        return U_PAIR[dtype], (2.0 ** -25 if f16 else 0.0)
    return U_MIXED[dtype], (2.0 ** -25 if f16 else 2.0 ** -24)


def _stats(x):
    d = x.shape[1]
    u = U32
    mean = x.mean(1, keepdim=True)
    c = x - mean
    var = (c * c).mean(1, keepdim=True)
    ve = var + LN_EPS
    rstd = ve.rsqrt()
    xhat = c * rstd
    e_mean = d * u * x.abs().mean(1, keepdim=True)
    e_c = e_mean + u * c.abs()
    e_var = ((2 * c.abs() + e_c) * e_c).mean(1, keepdim=True) + (d + 3) * u * ve
    e_rstd = rstd * (e_var / (2 * ve) + E_RSQ)
    e_xhat = rstd * e_c + (c.abs() + e_c) * e_rstd + u * xhat.abs()
    return rstd, xhat, e_rstd, e_xhat, ve


def ln_fwd_ref(x, gamma, beta, row_mul=1, rows=None):
    """(y, e_y) in float64: rows r * row_mul of x, r < rows."""
    rows = (x.shape[0] + row_mul - 1) // row_mul if rows is None else rows
    x = x[::row_mul][:rows].double()
    g, b = gamma.double().view(1, -1), beta.double().view(1, -1)
    _, xhat, _, e_xhat, _ = _stats(x)
    y = xhat * g + b
    return y, g.abs() * e_xhat + U32 * (xhat * g).abs() + U32 * y.abs()


def ln_bwd_ref(dy, x, gamma, resid=None, row_mul=1):
    """(out, e_out) in float64, [rows, d] dense (row r belongs at row r * row_mul of out32 / out16); dy holds the values the kernel
    reads (fp32, or the 16-bit ones widened)."""
    rows, d = dy.shape
    u = U32
    x = x[::row_mul][:rows].double()
    g = gamma.double().view(1, -1)
    rstd, xhat, e_rstd, e_xhat, _ = _stats(x)
    gg = dy.double() * g
    e_gg = u * gg.abs()
    s1 = gg.mean(1, keepdim=True)
    e_s1 = e_gg.mean(1, keepdim=True) + d * u * gg.abs().mean(1, keepdim=True)
    t = gg * xhat
    e_t = xhat.abs() * e_gg + (gg.abs() + e_gg) * e_xhat + u * t.abs()
    s2 = t.mean(1, keepdim=True)
    e_s2 = e_t.mean(1, keepdim=True) + d * u * t.abs().mean(1, keepdim=True)
    p = xhat * s2
    e_p = s2.abs() * e_xhat + (xhat.abs() + e_xhat) * e_s2 + u * p.abs()
    inner = gg - s1 - p
    e_in = e_gg + e_s1 + e_p + 2 * u * (gg.abs() + s1.abs() + p.abs())
    dx = rstd * inner
    e_dx = inner.abs() * e_rstd + (rstd + e_rstd) * e_in + u * dx.abs()
    if resid is None:
        return dx, e_dx
    r = resid[::row_mul][:rows].double()
    return dx + r, e_dx + u * (dx.abs() + r.abs())


def bound(ref, e, dtype, fmt=0):
    ur, uf = out_rounding(dtype, fmt)
    return ur * (ref.abs() + e) + uf + e


def var_plus_eps(x):
    """The values the device's rsqrtf sees (float64)."""
    return _stats(x.double())[4]


# ------------------------------------------------------------------------------------------------ plain fp32 evaluation (host)
def sum_sequential(t):
    acc = torch.zeros(t.shape[0], dtype=t.dtype)
    for j in range(t.shape[1]):
        acc = acc + t[:, j]
    return acc.view(-1, 1)


def sum_pairwise(t):
    n = 1
    while n < t.shape[1]:
        n *= 2
    t = torch.nn.functional.pad(t, (0, n - t.shape[1]))
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t


def sum_wave(t):
    """The kernels' order: lane l of 64 holds columns (i 64 + l) 4 .. + 3 of chunk i, adds ((v0 + v1) + v2) + v3 of each chunk to its
    partial sum, then a butterfly over the lanes (xor 32, 16, .., 1)."""
    rows, d = t.shape
    nv = (d + 255) // 256
    v = torch.nn.functional.pad(t, (0, nv * 256 - d)).view(rows, nv, 64, 4)
    s = torch.zeros(rows, 64, dtype=t.dtype)
    for i in range(nv):
        s = s + (((v[:, i, :, 0] + v[:, i, :, 1]) + v[:, i, :, 2]) + v[:, i, :, 3])
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, :1]


SUMS = {"sequential": sum_sequential, "pairwise": sum_pairwise, "wave": sum_wave}
MUTATIONS = ["var_d_minus_1", "no_eps", "mean_padded", "no_s1", "no_s2", "no_gamma_in_sums", "resid_twice", "neighbour_row"]


def _stats32(x, total, mut):
    d = x.shape[1]
    dm = float((d + 255) // 256 * 256) if mut == "mean_padded" else float(d)
    mean = total(x) / torch.tensor(dm)
    c = x - mean
    var = total(c * c) / torch.tensor(float(d - 1 if mut == "var_d_minus_1" else d))
    rstd = torch.rsqrt(var if mut == "no_eps" else var + torch.tensor(LN_EPS))
    return c * rstd, rstd


def ln_fwd_fp32(x, gamma, beta, total=sum_sequential, mut=None):
    """The forward in plain fp32 torch on the host (one rounding per operation), sums taken by `total`; `mut`: one of MUTATIONS."""
    xhat, _ = _stats32(x.float(), total, mut)
    y = xhat * gamma.view(1, -1) + beta.view(1, -1)
    return torch.roll(y, 1, 0) if mut == "neighbour_row" else y


def ln_bwd_fp32(dy, x, gamma, resid=None, total=sum_sequential, mut=None):
    d = x.shape[1]
    xhat, rstd = _stats32(x.float(), total, mut)
    gg = dy.float() * gamma.view(1, -1)
    insum = dy.float() if mut == "no_gamma_in_sums" else gg
    s1 = total(insum) / torch.tensor(float(d))
    s2 = total(insum * xhat) / torch.tensor(float(d))
    if mut == "no_s1":
        s1 = torch.zeros_like(s1)
    if mut == "no_s2":
        s2 = torch.zeros_like(s2)
    o = rstd * (gg - s1 - xhat * s2)
    if resid is not None:
        o = o + resid
        if mut == "resid_twice":
            o = o + resid
    return torch.roll(o, 1, 0) if mut == "neighbour_row" else o


# ------------------------------------------------------------------------------------------------ formats
def scaled(x, scale=None):
    """fl32(x s): the value every cast kernel encodes."""
    return x if scale is None else x * torch.tensor(scale, dtype=torch.float32, device=x.device)


def encode_plain(v, dtype):
    return v.to(dtype)


def encode_pair(v, dtype):
    """fp32 [rows, d] -> [rows, 2d] = [hi | lo]."""
    hi = v.to(dtype)
    return torch.cat([hi, (v - hi.float()).to(dtype)], dim=1).contiguous()


def encode(v, dtype, fmt):
    """fp32 [rows, d] in the format fmt (0 plain, 1 pair, 2 mixed; the unused quarter of a mixed row is zero)."""
    return encode_plain(v, dtype) if fmt == 0 else encode_pair(v, dtype) if fmt == 1 else encode_mixed(v, dtype)


def decode(p, fmt, d):
    """Float64 value of rows in the format fmt."""
    if fmt == 0:
        return p.double()
    if fmt == 1:
        return p[:, :d].double() + p[:, d:2 * d].double()
    return p[:, :d].double() + decode_lo8(p, d)


def planes(p, fmt, d):
    """The bits that belong to the value: int16 [rows, d] (plain), [rows, 2d] (pair) or [rows, d + d/2] (mixed: hi and the byte plane)."""
    w = p.view(torch.int16)
    return w[:, :d] if fmt == 0 else w[:, :2 * d] if fmt == 1 else w[:, :d + d // 2]


def cast_inputs(rows, d, limit=6e4, seed=0):
    """fp32 [rows, d] for the cast kernels: log-uniform magnitudes from 1e-6 to `limit` with random signs; row 0 sits on rounding ties
    of both 16-bit types (odd multiples of half an ulp, where round-to-nearest-EVEN decides), row 1 in the fp16 subnormal range
    (ties of its 2^-24 grid included), row 2 at the top of the range."""
    g = torch.Generator().manual_seed(31 * rows + d + seed)
    import math
    e = torch.rand(rows, d, generator=g) * (math.log(limit) - math.log(1e-6)) + math.log(1e-6)
    x = torch.exp(e) * torch.where(torch.rand(rows, d, generator=g) < 0.5, -1.0, 1.0)
    k = torch.arange(d, dtype=torch.float32)
    x[0, : d // 2] = 1.0 + (2 * (k[: d // 2] % 512) + 1) * 2.0 ** -11         # fp16 ties in [1, 2); the rest: bf16 ties
    x[0, d // 2:] = -(1.0 + (2 * (k[d // 2:] % 64) + 1) * 2.0 ** -8)
    if rows > 1:
        x[1] = (k % 2048 + 1) * 2.0 ** -25 * torch.where(k % 3 == 0, -1.0, 1.0)     # multiples of half an fp16 subnormal step
    if rows > 2:
        x[2] = limit * (1.0 - k / (4.0 * d))
    return x.clamp(-limit, limit).contiguous()


def pack_weight_ref(w, dtype, ld):
    """w [rows, cols] fp32 -> [rows, ld] of dtype, zero tail."""
    out = torch.zeros(w.shape[0], ld, dtype=dtype, device=w.device)
    out[:, :w.shape[1]] = w.to(dtype)
    return out


def pack_weight_t_ref(w, prefilled):
    """The transposed pack into `prefilled` [cols, ld] (a copy is returned): out[c][r] = round(w[r][c]); columns >= rows keep their bits."""
    out = prefilled.clone()
    out[:, :w.shape[0]] = w.t().to(prefilled.dtype)
    return out


def asymmetric_weight(rows, cols):
    """Integer-valued (exact in bf16 up to 256), different in every position of a 32 x 32 tile and not symmetric under a transpose."""
    r, c = torch.arange(rows).view(-1, 1), torch.arange(cols).view(1, -1)
    return ((r * 37 + c * 101 + (r // 32) * 7 + (c // 32) * 3) % 255 - 127).float()


def patch_image(B, R, seed=0):
    """Random fp32 pixels plus a ramp over (b, c, y, x), so that a swapped (ky, kx) or (gy, gx) cannot cancel."""
    g = torch.Generator().manual_seed(1009 * R + B + seed)
    b, c = torch.arange(B).view(B, 1, 1, 1), torch.arange(3).view(1, 3, 1, 1)
    y, x = torch.arange(R).view(1, 1, R, 1), torch.arange(R).view(1, 1, 1, R)
    return torch.randn(B, 3, R, R, generator=g) + 0.37 * y + 0.011 * x + 3.0 * c - 0.5 * (b % 7)


def patchify_ref(image, dtype, P, Kp):
    """image [B, 3, R, R] (any float type) -> [B G^2, Kp] of dtype by explicit index arithmetic."""
    B, _, R, _ = image.shape
    G, K = R // P, 3 * P * P
    dev = image.device
    row = torch.arange(B * G * G, device=dev).view(-1, 1)
    col = torch.arange(K, device=dev).view(1, -1)
    b, gy, gx = row // (G * G), (row // G) % G, row % G
    c, ky, kx = col // (P * P), (col % (P * P)) // P, col % P
    out = torch.zeros(B * G * G, Kp, dtype=dtype, device=dev)
    out[:, :K] = image[b, c, gy * P + ky, gx * P + kx].float().to(dtype)
    return out
