"""The stand-alone activation kernels (mvlpt_amd/csrc/activation.hip) at kernel level (-m gpu), through mvlpt_op_activation_fwd / _bwd,
against the float64 references and per-element bounds of tests/activation_ref.py.

Every case checks (1) every element under its derived bound, none exempt and no mean criterion, (2) the saved pre-activation, (3) a second
call bit for bit, (4) that the call without the saved u writes the same output, (5) that nothing outside the rows' own columns is written
(the padding of a pitched row, the unused quarter of a mixed pair).  Rows 1 / 77 / 130 (one lane group short of a workgroup, ragged, more
than one workgroup), widths 128 / 256, dense and dense + 8 pitches on both sides, fp16 and bf16, all three output formats.

The QuickGELU instantiation is held to the fused GEMM epilogues bit for bit (forward only: the derivative's contraction may differ
between two instantiations, so the backward is held to its float64 bound like the GELU one)."""
import ctypes as C

import pytest
import torch

from tests import activation_ref as R
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}
SENTINEL = 0x5a5a


def _E():
    from mvlpt_amd import engine
    return engine


def _L():
    from mvlpt_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _sentinel(M, width, dtype, dev):
    return torch.full((M, width), SENTINEL, dtype=torch.int16, device=dev).view(dtype)


def _pitched32(x, pad, dev):
    """fp32 rows at a pitch of N + pad floats, NaN in the padding"""
    out = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return out.to(dev)


def _untouched(out, fmt, N):
    """every 16-bit slot that is not part of the value still holds the sentinel"""
    raw = out.view(torch.int16)
    used = R.row_width(fmt, N) if fmt != "mixed" else N + N // 2
    return bool((raw[:, used:] == SENTINEL).all())


def _report(what, dtype, fmt, M, N, pad, got, ref, bound):
    nbad, ratio = R.violations(got, ref, bound)
    print(f"{what} {IDS[dtype]} {fmt} M={M} N={N} pitch +{pad}: worst per-element error / bound {ratio:.3f}")
    assert nbad == 0, (what, fmt, nbad, ratio)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("M,N", R.GRID)
def test_gelu_forward(M, N, fmt, dtype, dev):
    E = _E()
    u, _ = R.inputs(M, N)
    ref = R.fwd_reference(u, dtype, fmt)
    for pad in (0, 8):
        uin = _pitched32(u, pad, dev)
        width = R.row_width(fmt, N) + pad
        outs = []
        for save in (True, False, True):
            out = _sentinel(M, width, dtype, dev)
            u16 = _sentinel(M, N, dtype, dev) if save else None
            E.op_activation_fwd(uin, M, N, out, "gelu", R.FMT_CODE[fmt], ld_in=N + pad, ld_out=width if pad else 0, u16_out=u16)
            outs.append((out, u16))
        out, u16 = outs[0]
        _report("fwd", dtype, fmt, M, N, pad, R.decode(out, fmt, N).cpu(), *ref["out"])
        _report("fwd saved u", dtype, fmt, M, N, pad, u16.double().cpu(), *ref["u16"])
        assert _untouched(out, fmt, N), "the forward wrote outside its columns"
        assert torch.equal(out.view(torch.int16), outs[2][0].view(torch.int16)) and torch.equal(u16.view(torch.int16), outs[2][1].view(torch.int16))
        assert torch.equal(out.view(torch.int16), outs[1][0].view(torch.int16)), "the output depends on whether u is saved"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("M,N", R.GRID)
def test_gelu_backward(M, N, fmt, dtype, dev):
    E = _E()
    u, dA = R.inputs(M, N)
    u16 = u.to(dtype)
    ref, bound = R.bwd_reference(dA, u16, dtype, fmt)
    u16d = u16.to(dev)
    for pad in (0, 8):
        din = _pitched32(dA, pad, dev)
        width = R.row_width(fmt, N) + pad
        outs = []
        for _ in range(2):
            out = _sentinel(M, width, dtype, dev)
            E.op_activation_bwd(din, u16d, M, N, out, "gelu", R.FMT_CODE[fmt], ld_in=N + pad, ld_out=width if pad else 0)
            outs.append(out)
        got = R.decode(outs[0], fmt, N).cpu()
        _report("bwd", dtype, fmt, M, N, pad, got, ref, bound)
        assert bool((got[:, 10] == 0).all()), "dA = 0 must give 0"
        assert _untouched(outs[0], fmt, N), "the backward wrote outside its columns"
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "second run differs"
        assert torch.equal(u16d.cpu().view(torch.int16), u16.view(torch.int16)), "the saved pre-activation was written"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_quickgelu_backward_instantiation(fmt, dtype, dev):
    """The QuickGELU instantiation of the backward against gemm_ref's float64 QuickGELU' and its own measured function term."""
    E = _E()
    M, N = 130, 256
    u, dA = R.inputs(M, N)
    u16 = u.to(dtype)
    a, d = u16.double(), dA.double()
    ref = d * G.quick_gelu_grad(a)
    pre = G.E_FN_GELU_GRAD * G.gelu_grad_envelope(a) * d.abs() + 2.0 ** -24 * ref.abs()
    ur, uf = R.u_out(dtype, fmt)
    out = _sentinel(M, R.row_width(fmt, N), dtype, dev)
    E.op_activation_bwd(dA.to(dev), u16.to(dev), M, N, out, "quick_gelu", R.FMT_CODE[fmt])
    _report("bwd quick_gelu", dtype, fmt, M, N, 0, R.decode(out, fmt, N).cpu(), ref, ur * (ref.abs() + pre) + uf + pre)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
def test_quickgelu_forward_equals_the_fused_epilogue_bit_for_bit(dtype, dev):
    """op_gemm_ex(EPI_STORE32) + op_activation_fwd(quick_gelu) == op_gemm_ex(EPI_GELU / EPI_GELU_SPLIT, out_lo8 0 / 1): the activated
    output in all three formats and the saved pre-activation.  The format writers of the stand-alone pass are the epilogues'."""
    E = _E()
    M, N, K = 130, 256, 64
    pr = G.Problem("single", dtype, M, N, K)
    A, Bt, bias = pr.A.to(dev), pr.Bt.to(dev), pr.bias.to(dev)
    u32 = E.op_gemm_ex(A, Bt, G.EPI_STORE32, M, N, K, torch.empty(M, N, device=dev, dtype=torch.float32), bias=bias)
    for epi, lo8, fmt in ((G.EPI_GELU, 0, "single"), (G.EPI_GELU_SPLIT, 0, "pair"), (G.EPI_GELU_SPLIT, 1, "mixed")):
        width = R.row_width(fmt, N)
        fused, fused_u = torch.zeros(M, width, device=dev, dtype=dtype), torch.zeros(M, N, device=dev, dtype=dtype)
        E.op_gemm_ex(A, Bt, epi, M, N, K, fused, bias=bias, out2=fused_u, out_lo8=lo8)
        mine, mine_u = torch.zeros(M, width, device=dev, dtype=dtype), torch.zeros(M, N, device=dev, dtype=dtype)
        E.op_activation_fwd(u32, M, N, mine, "quick_gelu", R.FMT_CODE[fmt], u16_out=mine_u)
        assert bool(fused.view(torch.int16).any()), "the fused epilogue wrote nothing"
        assert torch.equal(mine.view(torch.int16), fused.view(torch.int16)), (fmt, "activated output differs from the fused epilogue")
        assert torch.equal(mine_u.view(torch.int16), fused_u.view(torch.int16)), (fmt, "saved pre-activation differs from the fused epilogue")


def test_malformed_arguments_are_refused_and_write_nothing(dev):
    L = _L()
    lib = L.lib
    M, N, dtype = 5, 128, torch.float16
    u32 = torch.zeros(M, N, device=dev)
    u16 = torch.zeros(M, N, device=dev, dtype=dtype)
    out = _sentinel(M, 2 * N + 8, dtype, dev)
    sav = _sentinel(M, N, dtype, dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ok = dict(dt=L.DT_F16, act=L.ACT_GELU, x=u32, ld_in=0, fmt=L.ACT_OUT_PAIR, out=out, ld_out=0, u=sav)
    bad = [dict(act=2), dict(act=-1), dict(fmt=3), dict(fmt=-1), dict(dt=L.DT_F32), dict(ld_out=2 * N - 8), dict(ld_out=2 * N + 4),
           dict(ld_in=N - 8), dict(ld_in=N + 4), dict(x=None), dict(out=None), dict(fmt=L.ACT_OUT_SINGLE, ld_out=N - 8)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.mvlpt_op_activation_fwd(a["dt"], a["act"], p(a["x"]), a["ld_in"], M, N, a["fmt"], p(a["out"]), a["ld_out"], p(a["u"]), None)
        assert rc == L.ERR_ARG and L.last_error(None), ("fwd", change, rc)
        rc = lib.mvlpt_op_activation_bwd(a["dt"], a["act"], p(a["x"]), a["ld_in"], p(u16), M, N, a["fmt"], p(a["out"]), a["ld_out"], None)
        assert rc == L.ERR_ARG and L.last_error(None), ("bwd", change, rc)
    rc = lib.mvlpt_op_activation_bwd(L.DT_F16, L.ACT_GELU, p(u32), 0, None, M, N, L.ACT_OUT_PAIR, p(out), 0, None)      # no saved u
    assert rc == L.ERR_ARG
    for Mb, Nb in ((0, N), (M, 0), (M, N + 4)):
        assert lib.mvlpt_op_activation_fwd(L.DT_F16, L.ACT_GELU, p(u32), 0, Mb, Nb, L.ACT_OUT_PAIR, p(out), 0, None, None) == L.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL).all()) and bool((sav.view(torch.int16) == SENTINEL).all()), "a refused call wrote"
    # ... and the legal call next to them goes through
    assert lib.mvlpt_op_activation_fwd(L.DT_F16, L.ACT_GELU, p(u32), 0, M, N, L.ACT_OUT_PAIR, p(out), 2 * N + 8, p(sav), None) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16)[:, :2 * N] == 0).all()) and bool((out.view(torch.int16)[:, 2 * N:] == SENTINEL).all())
