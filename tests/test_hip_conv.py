"""Kernel-level tests of the convolutional tower (-m gpu): mvlpt_op_conv2d, avgpool2x2, nchw_to_nhwc8, attnpool_tokens and
attnpool_query against float64 on fp16-exact inputs.  Every bound is derived in tests/resnet_ref.py from float64 magnitudes (the
accumulation term holds for any summation order); nothing is fitted to what the device returns.  Each test prints its worst
error / bound ratio.  Outputs sit between sentinel-filled guard regions that must come back untouched."""
import numpy as np
import pytest
import torch

from tests import resnet_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = 256, 12345.0


def guarded(shape, fill=float("nan")):
    """(flat buffer, view of `shape` in its middle): GUARD sentinel halves on either side, the view prefilled with `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float16)
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def rnd16(gen, shape, std=1.0):
    return (torch.randn(shape, generator=gen) * std).half()


def check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound).max())
    print(f"{what}: worst error / bound {ratio:.3f} (max error {float(err.max()):.3e})")
    assert torch.isfinite(got).all()
    assert ratio <= 1.0, f"{what}: error over the derived bound by {ratio:.3f}"


def run_conv(B, H, W, cin, cout, k, stride=1, relu=False, resid=False, negative_scale=False, seed=0):
    from mvlpt_amd.engine import conv_out_size, op_conv2d, op_pack_conv_weight
    g = torch.Generator().manual_seed(seed + 1000 * k + cin + cout)
    x = rnd16(g, (B, H, W, cin))
    w = rnd16(g, (cout, cin, k, k), (2.0 / (cin * k * k)) ** 0.5)
    scale = 1.0 + 0.3 * torch.randn(cout, generator=g)
    if negative_scale:
        scale = scale * torch.where(torch.arange(cout) % 3 == 0, -1.0, 1.0)
    shift = 0.2 * torch.randn(cout, generator=g)
    ho, wo = conv_out_size(H, k, stride), conv_out_size(W, k, stride)
    r = rnd16(g, (B, ho, wo, cout)) if resid else None
    ref, bound = R.conv_reference(x, w.float(), scale, shift, stride=stride, relu=relu, resid=r)
    buf, out = guarded((B, ho, wo, cout))
    wp = op_pack_conv_weight(w.float().to(DEV))
    assert wp.shape == (cout, R.conv_kp(k, cin))
    op_conv2d(x.to(DEV), wp, scale.to(DEV), shift.to(DEV), k, stride, relu, None if r is None else r.to(DEV), out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf), "the kernel wrote outside its output"
    if relu:
        assert bool((out >= 0).all())
        assert ref.numel() < 64 or bool((ref == 0).any()), "signed inputs: ReLU must have something to cut"
    check(out, ref, bound, f"conv k{k} s{stride} {(B, H, W, cin, cout)} relu {relu} resid {resid}")


@pytest.mark.parametrize("shape", [(1, 1, 1, 8, 8), (3, 3, 3, 8, 8), (2, 5, 7, 16, 40), (1, 56, 56, 64, 64)])
def test_conv3x3(shape):
    run_conv(*shape, k=3, relu=True)


@pytest.mark.parametrize("shape,resid", [((2, 3, 3, 8, 16), False), ((2, 3, 3, 32, 16), False), ((2, 3, 3, 40, 16), False),
                                         ((2, 7, 7, 2048, 512), False), ((2, 7, 7, 512, 2048), True)])
def test_conv1x1(shape, resid):
    """Cin below one K-step (32), exactly one, one + 8; the two stage-4 shapes, the second with residual + ReLU."""
    run_conv(*shape, k=1, relu=resid, resid=resid)


@pytest.mark.parametrize("shape", [(1, 8, 8, 16, 16), (1, 5, 13, 16, 16)])
@pytest.mark.parametrize("k", [1, 3])
def test_conv_one_tile_and_one_pixel_more(shape, k):
    """M = 64 output pixels is exactly one workgroup tile; M = 65 puts one pixel into a second, otherwise masked, tile."""
    assert shape[1] * shape[2] in (64, 65)
    run_conv(*shape, k=k, relu=True)


@pytest.mark.parametrize("shape", [(1, 6, 6, 8, 8), (1, 7, 5, 8, 32)])
def test_conv3x3_stride2(shape):
    run_conv(*shape, k=3, stride=2, relu=True)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("resid", [False, True])
def test_conv_epilogue(relu, resid):
    run_conv(2, 6, 5, 24, 48, k=3, relu=relu, resid=resid, negative_scale=True, seed=7)


@pytest.mark.parametrize("prefill", [0.0, float("nan")])
def test_stem_conv_on_the_padded_image(prefill):
    """The image's 3 channels travel as 8: the layout kernel must WRITE zeros into channels 3..7 (a buffer full of NaN shows it), and the
    weight's padded channels are zero, so the stride-2 stem conv sees exactly the 3-channel convolution."""
    from mvlpt_amd.engine import op_conv2d, op_nchw_to_nhwc8, op_pack_conv_weight
    g = torch.Generator().manual_seed(11)
    B, Rr, cout = 2, 10, 16
    image = torch.randn(B, 3, Rr, Rr, generator=g)
    w = rnd16(g, (cout, 3, 3, 3), (2.0 / 27) ** 0.5)
    scale, shift = 1.0 + 0.3 * torch.randn(cout, generator=g), 0.2 * torch.randn(cout, generator=g)
    ibuf, img8 = guarded((B, Rr, Rr, 8), prefill)
    op_nchw_to_nhwc8(image.to(DEV), out=img8)
    torch.cuda.synchronize()
    assert guards_intact(ibuf)
    assert torch.equal(img8[..., :3].cpu(), image.permute(0, 2, 3, 1).half()) and bool((img8[..., 3:] == 0).all())
    wp = op_pack_conv_weight(w.float().to(DEV))
    assert wp.shape == (cout, R.conv_kp(3, 8)) and bool((wp.view(cout, -1)[:, :72].view(cout, 9, 8)[:, :, 3:] == 0).all())
    buf, out = guarded((B, 5, 5, cout))
    op_conv2d(img8, wp, scale.to(DEV), shift.to(DEV), 3, 2, True, out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    ref, bound = R.conv_reference(image.permute(0, 2, 3, 1).half(), w.float(), scale, shift, stride=2, relu=True, cin_pad=8)
    check(out, ref, bound, f"stem conv on the padded image (prefill {prefill})")


def asymmetric_weight(cout, cin, k):
    n, c, ky, kx = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(k), torch.arange(k), indexing="ij")
    return ((7 * n + 3 * c + 5 * ky + 11 * kx) % 31 - 15).float()


def test_identity_activations_1x1_bit_exact():
    """A = I: pixel m carries a one in channel m, so y[m, n] = w[n, m] * 2 + 3 exactly — any slip in the MFMA fragment map (rows for
    columns, a k-slice in the wrong lane group) moves an entry of the asymmetric weight."""
    from mvlpt_amd.engine import op_conv2d, op_pack_conv_weight
    cin, cout = 40, 24
    x = torch.eye(cin).half().view(1, 5, 8, cin)
    w = asymmetric_weight(cout, cin, 1)
    scale, shift = torch.full((cout,), 2.0), torch.full((cout,), 3.0)
    out = op_conv2d(x.to(DEV), op_pack_conv_weight(w.to(DEV)), scale.to(DEV), shift.to(DEV), 1)
    want = (w.view(cout, cin).T * 2 + 3).half().view(1, 5, 8, cout)
    assert torch.equal(out.cpu(), want)


def test_impulse_activations_3x3_bit_exact():
    """Image b is an impulse in channel b at the centre of a 3 x 3 map: y[b, oy, ox, n] = w[n, b, 2 - oy, 2 - ox] exactly."""
    from mvlpt_amd.engine import op_conv2d, op_pack_conv_weight
    cin, cout = 16, 24
    x = torch.zeros(cin, 3, 3, cin)
    x[torch.arange(cin), 1, 1, torch.arange(cin)] = 1
    w = asymmetric_weight(cout, cin, 3)
    out = op_conv2d(x.half().to(DEV), op_pack_conv_weight(w.to(DEV)), torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV), 3)
    want = w.flip(2, 3).permute(1, 2, 3, 0).half()          # [b = c, oy, ox, n]
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 6, 10, 24), (1, 56, 56, 64)])
def test_avgpool(shape):
    from mvlpt_amd.engine import op_avgpool2x2
    g = torch.Generator().manual_seed(3)
    x = rnd16(g, shape)
    B, H, W, c = shape
    buf, out = guarded((B, H // 2, W // 2, c))
    op_avgpool2x2(x.to(DEV), out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    ref, bound = R.avgpool_reference(x)
    check(out, ref, bound, f"avgpool {shape}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("Rr", [2, 64])
def test_nchw_to_nhwc8(dtype, Rr):
    from mvlpt_amd.engine import op_nchw_to_nhwc8
    g = torch.Generator().manual_seed(4)
    image = torch.randn(3, 3, Rr, Rr, generator=g).to(dtype)
    buf, out = guarded((3, Rr, Rr, 8))
    op_nchw_to_nhwc8(image.to(DEV), out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    assert torch.equal(out[..., :3].cpu(), image.permute(0, 2, 3, 1).half())
    assert bool((out[..., 3:] == 0).all())


@pytest.mark.parametrize("B,HW,E", [(1, 1, 512), (3, 4, 512), (2, 9, 512), (2, 49, 2048)])
def test_attnpool_tokens(B, HW, E):
    from mvlpt_amd.engine import op_attnpool_tokens
    g = torch.Generator().manual_seed(5)
    x, pos = rnd16(g, (B, HW, E)), torch.randn(HW + 1, E, generator=g) * E ** -0.5
    buf, out = guarded((B, HW + 1, E))
    op_attnpool_tokens(x.to(DEV), pos.to(DEV), out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    ref, bound = R.tokens_reference(x, pos)
    check(out, ref, bound, f"attnpool tokens {(B, HW, E)}")


@pytest.mark.parametrize("T", [2, 5, 10, 50, 145])
@pytest.mark.parametrize("E", [512, 2048])
@pytest.mark.parametrize("B", [1, 3])
def test_attnpool_query(T, E, B):
    from mvlpt_amd.engine import op_attnpool_query
    g = torch.Generator().manual_seed(6 + T)
    q, kv = rnd16(g, (B, E)), rnd16(g, (B, T, 2 * E), 0.5)
    # head 0 of the last image: one key whose score is 80 above the rest (|q|^2 = 64, k = 10 q: 64 * 10 / 8): without the max
    # subtraction exp(80) = 5.5e34 times |v| leaves the fp16 range of the output and loses the small weights
    q[B - 1, :64] = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0).half()
    kv[B - 1, :, :64] = rnd16(g, (T, 64), 0.05)
    kv[B - 1, T - 1, :64] = q[B - 1, :64] * 10
    buf, out = guarded((B, E))
    op_attnpool_query(q.to(DEV), kv.to(DEV), out=out)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    ref, bound = R.query_reference(q, kv)
    assert float((ref[B - 1, :64] - kv[B - 1, T - 1, E:E + 64].double()).abs().max()) < 1e-6, "the dominant key owns that head"
    check(out, ref, bound, f"attnpool query T {T} E {E} B {B}")


def test_refusals_leave_the_output_alone():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import op_conv2d_raw
    x = torch.zeros(1, 4, 4, 16, device=DEV, dtype=torch.float16)
    w = torch.zeros(16, 800, device=DEV, dtype=torch.float16)
    s = torch.ones(16, device=DEV)
    buf, out = guarded((1, 4, 4, 16), SENTINEL)
    cases = [
        (dict(Cin=12), _lib.ERR_UNSUPPORTED),                 # Cin % 8
        (dict(Cout=12), _lib.ERR_UNSUPPORTED),
        (dict(k=5), _lib.ERR_UNSUPPORTED),
        (dict(k=1, stride=2), _lib.ERR_UNSUPPORTED),          # stride 2 belongs to the 3 x 3 stem conv only
        (dict(stride=3), _lib.ERR_UNSUPPORTED),
        (dict(x=None), _lib.ERR_ARG), (dict(w=None), _lib.ERR_ARG), (dict(scale=None), _lib.ERR_ARG), (dict(y=None), _lib.ERR_ARG),
        (dict(B=0), _lib.ERR_ARG),
    ]
    for change, code in cases:
        a = dict(x=x, w=w, scale=s, shift=s, resid=None, y=out, B=1, H=4, W=4, Cin=16, Cout=16, k=3, stride=1, relu=0)
        a.update(change)
        assert op_conv2d_raw(**a) == code, change
        assert _lib.last_error(None)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()), "a refused call must not touch the device"
    assert _lib.lib.mvlpt_op_avgpool2x2(None, None, 1, 2, 2, 8, None) == _lib.ERR_ARG
    assert _lib.lib.mvlpt_op_avgpool2x2(x.data_ptr(), out.data_ptr(), 1, 4, 4, 12, None) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.mvlpt_op_attnpool_query(x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 146, 64, None) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.mvlpt_op_nchw_to_nhwc8(None, 0, None, 1, 2, None) == _lib.ERR_ARG
    assert _lib.lib.mvlpt_op_attnpool_tokens(None, None, None, 1, 1, 64, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
