"""The LayerNorm kernels at kernel level (-m gpu) through mvlpt_op_layernorm_fwd_ex / _bwd_ex, with every argument the towers set,
against the float64 reference and the derived per-element bound of tests/norm_format_ref.py (rows of six kinds mixed in every tensor).

Every case (1) asserts its kernel, NV and grid through mvlpt_op_layernorm_route, so a moved threshold fails here instead of silently
moving the coverage, (2) writes into buffers prefilled with a sentinel between sentinel guards: the guards, the rows between the strided
rows of a row_mul > 1 call and the unused quarter of a mixed row must come back untouched, (3) checks every element against its own
bound (pair and mixed outputs through the reference decoders) and prints the worst error / bound, (4) runs twice and compares bit for
bit.  The backward's 16-bit copy must be the encoding of the fp32 output the same call returned, bit for bit (plain: round16; pair and
mixed: both planes).  The float64 reference is computed on the device; its last rows are checked against the host's.

Instantiations reached (TO / T = output type, TDY = type of dy, NV = float4 per lane):
  test_fwd_direct        ln_fwd_kernel<float | f16 | bf16>, split 0 / 1 / 2, rows {1, 3, 4, 5, 203} x d {4 .. 2048}; row_mul 5 at rows 5, 203
  test_fwd_stream_32cu   ln_fwd_stream_kernel<float | f16 | bf16, NV> with NV 2 / 3 / 4 / 8 / 8 at d 260 / 768 / 1024 / 1280 / 2048 on a
                         32-CU stream (256 workgroups = 1024 waves): rows 4096 (four rounds exactly), 4097 (one wave runs a fifth row),
                         5123 (ragged), all seven outputs each, and row_mul 5 at 4097 x 260
  test_bwd_direct        ln_bwd_kernel<float, f16 | bf16> with split 0 / 1 / 2, ln_bwd_kernel<f16, f16> and <bf16, bf16> (split 0); without
                         resid; without out16; in place; row_mul 5 at rows 5, 203
  test_bwd_stream_32cu   ln_bwd_stream_kernel<float, f16 | bf16, NV> with split 0 / 1 / 2, <f16, f16, NV> and <bf16, bf16, NV> (split 0) for each
                         NV and row count as above; without resid; without out16; in place; row_mul 5 at 4097 x 260
  test_default_stream    the whole device at d = 260 (NV 2): rows 4096 (one pass, no prefetch) and 32 * CUs + 5 (some waves run two rows)
  test_refusals          d % 4, d = 2052, unknown dtypes and splits leave the guarded outputs untouched; rows = 0 writes nothing
LnFwdArgs::row_idx / LnBwdArgs::row_idx have no caller and no entry: not tested.
"""
import pytest
import torch

from tests import norm_format_ref as N

pytestmark = pytest.mark.gpu

GUARD = 4096            # bytes on either side of every output
FILL = 0x5a
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ALL_OUTPUTS = [(F32, 0)] + [(t, f) for t in (F16, BF16) for f in (0, 1, 2)]


def _E():
    from mvlpt_amd import engine
    return engine


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def stream32(dev):
    E = _E()
    st = E.partition_stream(dev, 0, 32)
    assert E.device_cus(dev) >= 32 and E.stream_cus(st) == 32
    return st


def guarded(rows, width, dtype, dev):
    """(whole byte buffer, its [rows, width] middle of `dtype`), every byte FILL."""
    n = rows * width * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(rows, width)


def guards_intact(buf):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


def untouched(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


def between_rows_untouched(t, row_mul, rows):
    """Rows of `t` that are not r * row_mul, r < rows, still hold the sentinel."""
    keep = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
    keep[torch.arange(rows, device=t.device) * row_mul] = False
    return untouched(t[keep]) if bool(keep.any()) else True


def expected_route(rows, d, cus):
    if rows < 4096:
        return (0, 8, (rows + 3) // 4)
    nv = (d + 255) // 256
    return (1, 2 if nv <= 2 else nv if nv <= 4 else 8, min((rows + 3) // 4, 8 * cus))


def device_reference(fn, host_fn, what):
    """The float64 reference on the device, its last rows checked against the host's (to a thousandth of the bound)."""
    ref, e = fn()
    h_ref, h_e = host_fn()
    k = h_ref.shape[0]
    assert bool(((ref[-k:].cpu() - h_ref).abs() <= 1e-3 * h_e + 1e-300).all()), f"{what}: device and host float64 references differ"
    return ref, e


def check(got, ref, e, dtype, fmt, what):
    nbad, ratio = N.violations(got, ref, N.bound(ref, e, dtype, fmt))
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert nbad == 0, (what, nbad, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ forward
def fwd_case(rows, d, row_mul, outputs, dev, cus):
    E = _E()
    assert E.op_layernorm_route(rows, d) == expected_route(rows, d, cus), (rows, d)
    t = N.ln_inputs(rows * row_mul, d)
    x, g, b = (t[k].to(dev) for k in ("x", "gamma", "beta"))
    k = min(rows, 64)
    ref, e = device_reference(lambda: N.ln_fwd_ref(x, g, b, row_mul, rows),
                              lambda: N.ln_fwd_ref(t["x"][::row_mul][:rows][-k:], t["gamma"], t["beta"]), "forward")
    for dtype, fmt in outputs:
        width = d * (2 if fmt else 1)
        runs = []
        for _ in range(2):
            buf, y = guarded(rows, width, dtype, dev)
            E.op_layernorm_fwd_ex(x, g, b, y, rows, d, row_mul=row_mul, split=fmt)
            torch.cuda.current_stream().synchronize()
            assert guards_intact(buf), "the kernel wrote outside its output"
            runs.append(y)
        y = runs[0]
        assert torch.equal(y.view(torch.uint8), runs[1].view(torch.uint8)), "second run differs"
        if fmt == 2:
            assert untouched(y[:, d + d // 2:]), "the unused quarter of a mixed row was written"
        check(N.decode(y, fmt, d), ref, e, dtype, fmt, f"fwd rows={rows} d={d} row_mul={row_mul} {N.IDS[dtype]} split {fmt}")


@pytest.mark.parametrize("d", N.DIRECT_D)
@pytest.mark.parametrize("rows", N.DIRECT_ROWS)
def test_fwd_direct(rows, d, dev):
    cus = _E().stream_cus()
    fwd_case(rows, d, 1, ALL_OUTPUTS, dev, cus)
    if rows in (5, 203):
        fwd_case(rows, d, 5, ALL_OUTPUTS, dev, cus)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d", list(N.STREAM_D))
@pytest.mark.parametrize("rows", N.STREAM_ROWS)
def test_fwd_stream_32cu(rows, d, dev, stream32):
    with torch.cuda.stream(stream32):
        assert _E().op_layernorm_route(rows, d)[:2] == (1, N.STREAM_D[d])
        fwd_case(rows, d, 1, ALL_OUTPUTS, dev, 32)
        if (rows, d) == (4097, 260):
            fwd_case(rows, d, 5, ALL_OUTPUTS, dev, 32)
        torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------------------------------------ backward
def bwd_case(rows, d, row_mul, configs, dev, cus):
    """configs: (dtype, dy16, split, resid, out16, inplace) per launch."""
    E = _E()
    assert E.op_layernorm_route(rows, d) == expected_route(rows, d, cus), (rows, d)
    total = rows * row_mul
    t = N.ln_inputs(total, d)
    x, g, resid = (t[k].to(dev) for k in ("x", "gamma", "resid"))
    k = min(rows, 64)
    refs = {}
    for dtype, dy16, split, use_resid, want16, inplace in configs:
        dy_h = t["dy"][:rows].to(dtype) if dy16 else t["dy"][:rows]
        dy = dy_h.to(dev)
        key = (dtype if dy16 else F32, use_resid)
        if key not in refs:
            h_resid = t["resid"][::row_mul][:rows][-k:] if use_resid else None
            refs[key] = device_reference(lambda: N.ln_bwd_ref(dy.float(), x, g, resid if use_resid else None, row_mul),
                                         lambda: N.ln_bwd_ref(dy_h[-k:].float(), t["x"][::row_mul][:rows][-k:], t["gamma"], h_resid), "backward")
        ref, e = refs[key]
        width = d * (2 if split else 1)
        what = (f"bwd rows={rows} d={d} row_mul={row_mul} {N.IDS[dtype]} dy {'16-bit' if dy16 else 'fp32'} split {split}"
                f"{'' if use_resid else ' no resid'}{'' if want16 else ' no out16'}")
        runs = []
        for _ in range(2):
            b32, o32 = guarded(total, d, F32, dev)
            b16, o16 = guarded(total, width, dtype, dev) if want16 else (None, None)
            E.op_layernorm_bwd_ex(dy, x, g, o32, rows, d, dtype, resid=resid if use_resid else None, out16=o16, row_mul=row_mul, split=split)
            torch.cuda.current_stream().synchronize()
            assert guards_intact(b32) and (b16 is None or guards_intact(b16)), "the kernel wrote outside its outputs"
            runs.append((o32, o16))
        o32, o16 = runs[0]
        assert torch.equal(o32.view(torch.int32), runs[1][0].view(torch.int32)), "second run differs (out32)"
        assert between_rows_untouched(o32, row_mul, rows), "out32: a row between the strided rows was written"
        got = o32[::row_mul][:rows]
        check(got.double(), ref, e, F32, 0, what)
        if want16:
            assert torch.equal(o16.view(torch.int16), runs[1][1].view(torch.int16)), "second run differs (out16)"
            assert between_rows_untouched(o16, row_mul, rows), "out16: a row between the strided rows was written"
            r16 = o16[::row_mul][:rows]
            if split == 2:      # the fp8 conversion of the reference encoder is the host's
                assert untouched(r16[:, d + d // 2:]), "the unused quarter of a mixed row was written"
                want, have = N.encode(got.cpu(), dtype, 2), r16.cpu()
            else:
                want, have = N.encode(got.contiguous(), dtype, split), r16
            assert torch.equal(N.planes(have, split, d), N.planes(want, split, d)), f"{what}: out16 is not the encoding of out32"
        if inplace:
            assert use_resid
            buf = torch.full((total, d), float("nan"), device=dev)
            buf[::row_mul] = resid[::row_mul]          # the rows in between are not read either
            E.op_layernorm_bwd_ex(dy, x, g, buf, rows, d, dtype, resid=buf, out16=None, row_mul=row_mul, split=split)
            assert torch.equal(buf[::row_mul][:rows].view(torch.int32), got.view(torch.int32)), f"{what}: the in-place call differs"


def _direct_configs(dtype):
    return [(dtype, False, 0, True, True, True), (dtype, False, 1, True, True, False), (dtype, False, 2, True, True, False),
            (dtype, True, 0, True, True, False), (dtype, False, 0, False, True, False), (dtype, False, 1, True, False, False)]


@pytest.mark.parametrize("d", N.DIRECT_D)
@pytest.mark.parametrize("rows", N.DIRECT_ROWS)
def test_bwd_direct(rows, d, dev):
    cus = _E().stream_cus()
    bwd_case(rows, d, 1, _direct_configs(F16) + _direct_configs(BF16), dev, cus)
    if rows in (5, 203):
        bwd_case(rows, d, 5, [(F16, False, 0, True, True, True), (BF16, False, 2, True, True, False), (F16, False, 1, False, False, False),
                              (BF16, True, 0, True, True, False)], dev, cus)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d", list(N.STREAM_D))
@pytest.mark.parametrize("rows", N.STREAM_ROWS)
def test_bwd_stream_32cu(rows, d, dev, stream32):
    with torch.cuda.stream(stream32):
        assert _E().op_layernorm_route(rows, d)[:2] == (1, N.STREAM_D[d])
        bwd_case(rows, d, 1, _direct_configs(F16) + _direct_configs(BF16), dev, 32)
        if (rows, d) == (4097, 260):
            bwd_case(rows, d, 5, [(F16, False, 0, True, True, True), (BF16, False, 2, True, True, False), (F16, True, 0, False, True, False)],
                     dev, 32)
        torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------------------------------------ the whole device
@pytest.mark.parametrize("which", ["one_pass", "two_rows"])
def test_default_stream(which, dev):
    """The grid-stride kernels sized from the device's compute units: 4096 rows are one pass without a prefetch (1024 workgroups on 128
    compute units or more), 32 * CUs + 5 rows fill all 8 * CUs workgroups and give some waves a second row."""
    cus = _E().device_cus(dev)
    assert _E().stream_cus() == cus
    rows = 4096 if which == "one_pass" else max(4096, 32 * cus + 5)
    kind, nv, grid = _E().op_layernorm_route(rows, 260)
    assert (kind, nv) == (1, 2) and grid == min((rows + 3) // 4, 8 * cus)
    assert (grid * 4 >= rows) == (which == "one_pass" and cus >= 128)
    fwd_case(rows, 260, 1, [(F32, 0), (F16, 2), (BF16, 0)], dev, cus)
    bwd_case(rows, 260, 1, [(F16, False, 0, True, True, True), (BF16, False, 1, True, True, False)], dev, cus)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    E = _E()
    rows = 8
    for d, out_dtype, split in [(6, None, 0), (2052, None, 0), (260, 7, 0), (260, None, 3), (260, None, -1)]:
        t = N.ln_inputs(rows, d if d % 4 == 0 else d + 2)
        x, g, b, dy = (t[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
        buf, y = guarded(rows, 2 * d, F16, dev)
        with pytest.raises(RuntimeError):
            E.op_layernorm_fwd_ex(x, g, b, y, rows, d, split=split, out_dtype=out_dtype)
        b32, o32 = guarded(rows, d, F32, dev)
        with pytest.raises(RuntimeError):
            E.op_layernorm_bwd_ex(dy, x, g, o32, rows, d, F16 if out_dtype is None else out_dtype, out16=y, split=split)
        torch.cuda.synchronize()
        assert untouched(buf) and untouched(b32), (d, out_dtype, split)
        if split == 0 and out_dtype is None:
            with pytest.raises(RuntimeError):
                E.op_layernorm_route(rows, d)
    t = N.ln_inputs(rows, 260)
    x, g, b, dy = (t[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
    buf, y = guarded(rows, 520, F16, dev)
    b32, o32 = guarded(rows, 260, F32, dev)
    with pytest.raises(RuntimeError):           # a pair is 16-bit
        E.op_layernorm_fwd_ex(x, g, b, o32, rows, 260, split=1)
    with pytest.raises(RuntimeError):           # dy is fp32 or of the compute type
        E.op_layernorm_bwd_ex(dy.bfloat16(), x, g, o32, rows, 260, F16, out16=y)
    with pytest.raises(RuntimeError):
        E.op_layernorm_bwd_ex(dy, x, g, o32, rows, 260, F32, out16=y)
    with pytest.raises(RuntimeError):           # NULL pointers
        E.op_layernorm_fwd_ex(x, None, b, y, rows, 260)
    with pytest.raises(RuntimeError):
        E.op_layernorm_bwd_ex(dy, x, g, None, rows, 260, F16, out16=y)
    with pytest.raises(RuntimeError):
        E.op_layernorm_fwd_ex(x, g, b, y, rows, 260, row_mul=0)
    # rows = 0: success, nothing written
    E.op_layernorm_fwd_ex(x, g, b, y, 0, 260, split=1)
    E.op_layernorm_bwd_ex(dy, x, g, o32, 0, 260, F16, resid=x, out16=y, split=2)
    torch.cuda.synchronize()
    assert untouched(buf) and untouched(b32)
