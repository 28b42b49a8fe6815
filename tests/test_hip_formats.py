"""The kernels that define the operand formats, and the patch extraction, at kernel level (-m gpu): cast_to16_kernel, cast_split_kernel
(pair and mixed, with the device scale the towers pass), cast_to_f32_kernel, pack_weight_kernel, pack_weight_t_kernel, pack_weight8_kernel
and the three patchify kernels, against the bit-exact statements of tests/norm_format_ref.py.  Every comparison is torch.equal on the raw
16-bit or byte planes.  Outputs are prefilled with a sentinel and sit between sentinel guards; what a kernel does not own (the unused
quarter of a mixed row, the pitch padding of the transposed pack) must come back untouched.  Every patchify case asserts its kernel
through mvlpt_op_patchify_route."""
import pytest
import torch

from tests import gemm_ref as G
from tests import norm_format_ref as N

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0x5a
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
IDS = N.IDS


def _E():
    from mvlpt_amd import engine
    return engine


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def guarded(rows, width, dtype, dev):
    n = rows * width * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(rows, width)


def guards_intact(buf):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


def untouched(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


def bits(t):
    return t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------------ casts
def run_cast(x, dtype, fmt, scale, dev):
    """x fp32 [rows, d] on the host -> the device's encoding (host tensor), after the guard checks."""
    rows, d = x.shape
    sc = None if scale is None else torch.tensor([scale], dtype=F32, device=dev)
    buf, out = guarded(rows, d * (2 if fmt else 1), dtype, dev)
    _E().op_cast_ex(x.to(dev), out, rows, d, fmt=fmt, scale_dev=sc)
    torch.cuda.synchronize()
    assert guards_intact(buf), "the kernel wrote outside its output"
    if fmt == 2:
        assert untouched(out[:, d + d // 2:]), "the unused quarter of a mixed row was written"
    return out.cpu()


def check_cast(x, dtype, fmt, scale, dev):
    d = x.shape[1]
    v = N.scaled(x, scale)
    assert bool(torch.isfinite(v.to(dtype)).all()), "inputs stay inside the 16-bit range"
    want, have = N.encode(v, dtype, fmt), run_cast(x, dtype, fmt, scale, dev)
    hw, hh = N.planes(want, fmt, d), N.planes(have, fmt, d)
    assert torch.equal(hh[:, :d], hw[:, :d]), "hi plane"
    assert torch.equal(hh, hw), "lo plane" if fmt == 1 else "byte plane"
    return v


@pytest.mark.parametrize("d", [4, 256, 772])
@pytest.mark.parametrize("scale", [None, 2.0 ** -7, 3.0], ids=["noscale", "scale2^-7", "scale3"])
@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["plain", "pair", "mixed"])
@pytest.mark.parametrize("dtype", N.DTYPES, ids=["fp16", "bf16"])
def test_cast(dtype, fmt, scale, d, dev):
    """Magnitudes from 1e-6 to 6e4 (to 2e4 for fp16 under the scale of 3: the scaled value stays finite), a row of rounding ties, a row
    of fp16 subnormals, a row at the top of the range."""
    limit = 6e4 / 3 if (dtype == F16 and scale == 3.0) else 6e4
    x = N.cast_inputs(37, d, limit)
    v = check_cast(x, dtype, fmt, scale, dev)
    if dtype == BF16 and scale == 3.0 and d > 4:
        lo = (v - v.bfloat16().float()) * 2.0 ** N.LO8_EXP[BF16]
        assert float(lo.abs().max()) > 57344.0, "the bf16 mixed pair's clamp is reached"


@pytest.fixture(scope="module")
def wrap_input():
    rows, d = 2731, 772
    assert rows * (d // 4) > 2048 * 256 and rows * (d // 4) % 256 != 0        # more float4 than the capped grid has threads, ragged
    return N.cast_inputs(rows, d)


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["plain", "pair", "mixed"])
@pytest.mark.parametrize("dtype", N.DTYPES, ids=["fp16", "bf16"])
def test_cast_grid_wrap(dtype, fmt, wrap_input, dev):
    check_cast(wrap_input, dtype, fmt, None, dev)


@pytest.mark.parametrize("n", [1000 + 77, 2048 * 256 + 3 * 256 + 77])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["fp16", "bf16", "fp32"])
def test_cast_to_f32(dtype, n, dev):
    """Exact widening of every non-NaN 16-bit pattern (infinities and subnormals included), n not a multiple of 256, once below and once
    above the capped grid; fp32 input is a copy."""
    pat = (torch.arange(n, dtype=torch.int32) * 7 + 3) % 65536
    if dtype == F32:
        x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    else:
        x = (pat - 32768).to(torch.int16).view(dtype)
        x = torch.where(torch.isnan(x), torch.ones((), dtype=dtype), x)
    buf, out = guarded(1, n, F32, dev)
    _E().op_cast_to_f32(x.to(dev), out, n)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    assert torch.equal(bits(out.cpu().view(-1)), bits(x.float()))


# ------------------------------------------------------------------------------------------------ weight packs
@pytest.mark.parametrize("rows,cols,pad", [(33, 65, 0), (33, 65, 64), (1100, 1000, 0), (1100, 1000, 64)])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_pack_weight(dtype, rows, cols, pad, dev):
    """round16(w) at a pitch with a zero tail; 1100 x 1000 is more than 4096 x 256 elements (the capped grid wraps, ragged)."""
    if rows == 1100:
        assert rows * (cols + pad) > 4096 * 256
    w = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)) * 3
    buf, out = guarded(rows, cols + pad, dtype, dev)
    _E().op_pack_weight(w.to(dev), out, rows, cols, ld_out=cols + pad)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    assert torch.equal(bits(out.cpu()), bits(N.pack_weight_ref(w, dtype, cols + pad)))


@pytest.mark.parametrize("rows,cols", [(1, 1), (32, 32), (33, 65), (100, 37), (768, 3072)])
@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_pack_weight_t(dtype, pad, rows, cols, dev):
    """out[c][r] = w[r][c] through the 32 x 32 LDS tiles (ragged in both directions); the pitch padding is not written."""
    w = N.asymmetric_weight(rows, cols)
    buf, out = guarded(cols, rows + pad, dtype, dev)
    before = out.cpu()
    _E().op_pack_weight(w.to(dev), out, rows, cols, transposed=True, ld_out=rows + pad)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    have = out.cpu()
    assert torch.equal(have[:, :rows].float(), w.t()), "the transpose"
    assert torch.equal(bits(have), bits(N.pack_weight_t_ref(w, before))), "the pitch padding was written"
    if pad == 0:        # ld_out = 0 means dense
        buf2, out2 = guarded(cols, rows, dtype, dev)
        _E().op_pack_weight(w.to(dev), out2, rows, cols, transposed=True)
        assert torch.equal(bits(out2.cpu()), bits(have)) and guards_intact(buf2)


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("dtype", N.DTYPES, ids=["fp16", "bf16"])
def test_pack_weight_mixed_planes(dtype, transposed, dev):
    """Both planes of the mixed weight bit for bit, and its exponent.  The weight holds 16-bit values (what the towers' checkpoints are
    after their first rounding), so that the fp8 plane of the fp32 weight and of its 16-bit plane are the same statement."""
    g = torch.Generator().manual_seed(5)
    R_, K = 130, 256
    W = (torch.randn(R_, K, generator=g) * K ** -0.5).to(dtype)          # the packed weight [R, K]
    W[3, 5] = W.abs().max() * 1.5                                        # a lone maximum decides the exponent
    src = W.float().t().contiguous() if transposed else W.float()
    packed, e8 = _E().op_pack_weight_mixed(src.to(dev), dtype, transposed=transposed)
    assert e8 == G.w8_exponent(W.float())
    want, _ = G.pack_weight_mixed(W, e8)
    have = packed.cpu()
    assert have.shape == want.shape == (R_, K + K // 2)
    assert torch.equal(have[:, :K].view(torch.int16), want[:, :K].view(torch.int16)), "16-bit plane"
    assert torch.equal(bits(have[:, K:]), bits(want[:, K:])), "e4m3 plane"


# ------------------------------------------------------------------------------------------------ patchify
SCALAR, VEC, COPY16 = 0, 1, 2


def run_patchify(image, dtype, P, Kp, route, dev):
    """image: device tensor [B, 3, R, R]; the reference runs on the device (plain torch indexing)."""
    E = _E()
    B, _, R, _ = image.shape
    assert E.op_patchify_route(dtype, image.dtype, R, P) == route, (dtype, image.dtype, R, P)
    rows = B * (R // P) ** 2
    buf, out = guarded(rows, Kp, dtype, dev)
    E.op_patchify(image, out, B, R, P, Kp)
    torch.cuda.synchronize()
    assert guards_intact(buf), "the kernel wrote outside its output"
    want = N.patchify_ref(image, dtype, P, Kp)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("extra", [0, 64], ids=["Kp=3PP", "Kp=3PP+64"])
@pytest.mark.parametrize("R,P", [(16, 8), (64, 16), (64, 32)])
@pytest.mark.parametrize("dtype", N.DTYPES, ids=["fp16", "bf16"])
def test_patchify_vec_and_copy16(dtype, R, P, extra, B, dev):
    img = N.patch_image(B, R).to(dev)
    run_patchify(img, dtype, P, 3 * P * P + extra, VEC, dev)
    run_patchify(img.to(dtype), dtype, P, 3 * P * P + extra, COPY16, dev)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", N.DTYPES, ids=["fp16", "bf16"])
def test_patchify_scalar(dtype, B, dev):
    other = BF16 if dtype == F16 else F16
    for src in (F32, dtype, other):       # ViT-L/14's geometry: 588 columns and a zero tail up to 640
        run_patchify(N.patch_image(B, 28).to(dev).to(src), dtype, 14, 640, SCALAR, dev)
    run_patchify(N.patch_image(B, 64).to(dev).to(other), dtype, 16, 768, SCALAR, dev)          # an image of the other 16-bit type
    run_patchify(N.patch_image(B, 64).to(dev).to(other), dtype, 16, 768 + 64, SCALAR, dev)
    # 3 P (R / 8) 16 bytes = 73728 > 64 KB: the 16-byte copy does not fit its LDS and the scalar kernel takes over
    run_patchify(N.patch_image(B, 384).to(dev).to(dtype), dtype, 32, 3072, SCALAR, dev)


@pytest.fixture(scope="module")
def big_image():
    return N.patch_image(223, 224)


@pytest.mark.parametrize("route", [SCALAR, VEC], ids=["scalar", "vec"])
def test_patchify_grid_wrap(route, big_image, dev):
    """The smallest batch at (224, 16) whose 8-column work items exceed the capped grid, with a ragged remainder (40 of the 8192
    workgroups, resp. 6.5 of the 16384, run a second item): 112 images over 8192 x 256 (scalar: a bf16 image into fp16), 223 over
    16384 x 256 (vec: an fp32 image into bf16)."""
    B, cap = (112, 8192 * 256) if route == SCALAR else (223, 16384 * 256)
    items = B * 196 * 96
    assert (B - 1) * 196 * 96 <= cap < items < cap + cap // 8       # the smallest such batch; only a few workgroups wrap
    img = big_image[:B].to(dev)
    run_patchify(img.to(BF16) if route == SCALAR else img, F16 if route == SCALAR else BF16, 16, 768, route, dev)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    E = _E()
    x = torch.randn(8, 260, device=dev)
    buf, out = guarded(8, 520, F16, dev)
    for kw in [dict(rows=8, d=6), dict(rows=8, d=260, fmt=3), dict(rows=8, d=260, fmt=-1), dict(rows=8, d=260, dtype=7),
               dict(rows=8, d=260, dtype=0), dict(rows=-1, d=260)]:
        with pytest.raises(RuntimeError):
            E.op_cast_ex(x, out, **kw)
    with pytest.raises(RuntimeError):
        E.op_cast_ex(None, out, 8, 260)
    with pytest.raises(RuntimeError):
        E.op_cast_to_f32(x, out, 8, in_dtype=5)
    with pytest.raises(RuntimeError):
        E.op_pack_weight(x, out, 8, 260, dtype=9)
    with pytest.raises(RuntimeError):
        E.op_pack_weight(x, out, 8, 260, ld_out=256)                   # shorter than a row
    with pytest.raises(RuntimeError):
        E.op_pack_weight(x, out, 8, 260, transposed=True, ld_out=4)
    img = torch.randn(1, 3, 32, 32, device=dev)
    for kw in [dict(R=32, P=8, Kp=196), dict(R=32, P=12, Kp=432), dict(R=32, P=8, Kp=184), dict(R=32, P=8, Kp=192, dtype=0),
               dict(R=32, P=8, Kp=192, image_dtype=4), dict(R=32, P=0, Kp=192)]:
        with pytest.raises(RuntimeError):
            E.op_patchify(img, out, 1, **kw)
    with pytest.raises(RuntimeError):
        E.op_patchify_route(F16, F32, 32, 12)
    with pytest.raises(RuntimeError):
        E.op_patchify_route(F32, F32, 32, 8)
    E.op_cast_ex(x, out, 0, 260, fmt=2)                                 # rows = 0: success, nothing written
    E.op_cast_to_f32(x.half(), out, 0)
    torch.cuda.synchronize()
    assert untouched(buf)
