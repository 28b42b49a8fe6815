"""The GEMM references, decoders and bounds of tests/gemm_ref.py, checked without a GPU: a plain fp32 host GEMM + epilogue stays inside
every per-element bound at the shapes of tests/test_hip_gemm_matrix.py, one perturbed element falls outside, the pair decoders round-trip,
and the one measured constant (the QuickGELU factor's fp32 error) is re-measured."""
import pytest
import torch

from oracle import clip_oracle as O
from tests import gemm_ref as R

# (route, format, K) at the ragged M.  The bounds are elementwise and every row is computed alike, so the other two M values of the GPU
# matrix (which exist for the kernels' tile edges) add nothing on the host.
CASES = [(r, f, K) for r in R.ROUTES32 for f in R.FORMATS if not (r == "pc" and f == "single") for K in R.K_VALUES[f]]
CASES += [("phased", f, R.PHASED32[f][2]) for f in R.PHASED32]


def _shape(route, fmt, K):
    if route == "phased":
        return R.PHASED32[fmt]
    return R.ROUTES32[route][0], R.ROUTES32[route][3], K


def _out_lo8(fmt):
    return 1 if fmt == "mixed" else 0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("route,fmt,K", CASES)
def test_fp32_host_gemm_is_inside_every_bound(route, fmt, K, dtype):
    M, N, K = _shape(route, fmt, K)
    # the big shapes: a slice of rows is the same check (rows are independent) at a fraction of the float64 matmul
    M = min(M, 600)
    pr = R.Problem(fmt, dtype, M, N, K)
    acc, S = pr.products()
    for epi in R.LEGAL_EPIS[fmt]:
        ref = R.reference(epi, acc, S, pr.k_eff, dtype, bias=None if epi in (3, 6) else pr.bias, resid=pr.resid, aux=pr.aux, out_lo8=_out_lo8(fmt))
        got = R.fp32_host(pr, epi, out_lo8=_out_lo8(fmt))
        for which, (r, b) in ref.items():
            g = got[which]
            nbad, ratio = R.violations(g, r, b)
            assert nbad == 0, (epi, which, nbad, ratio)
            assert R.relerr(g, r) < R.maxnorm_tol(fmt, dtype, epi, which)
            # one element moved by four times its bound is caught, wherever it sits (the smallest-magnitude element included)
            idx = int(r.abs().argmin())
            p = g.clone().view(-1)
            p[idx] = r.view(-1)[idx] + 4 * b.reshape(-1)[idx] + 1e-300
            assert R.violations(p.view_as(g), r, b)[0] == 1


def test_bound_catches_a_wrong_gelu_grad_factor_at_very_negative_u():
    """The case a max-norm misses: QuickGELU'(u) at u << 0 is tiny, so a wrong factor there hides under max|ref|."""
    dtype = torch.float16
    pr = R.Problem("single", dtype, 300, 256, 128)
    acc, S = pr.products()
    aux = pr.aux.clone()
    aux[7, 11] = -9.0
    ref, b = R.reference(3, acc, S, pr.k_eff, dtype, aux=aux)["out"]
    good = (acc.float() * O.quick_gelu_grad(aux.float())).to(dtype).double()
    assert R.violations(good, ref, b)[0] == 0
    bad = good.clone()
    bad[7, 11] = float((acc[7, 11] * R.quick_gelu_grad(torch.tensor(-8.0, dtype=torch.float64))).to(dtype))     # the neighbour's factor
    assert R.relerr(bad, ref) < R.TOL[dtype]          # invisible to the max-norm
    assert R.violations(bad, ref, b)[0] == 1


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
def test_decoders_round_trip(dtype):
    from mvlpt_amd import engine as E
    g = torch.Generator().manual_seed(3)
    x = torch.randn(130, 256, generator=g) * torch.logspace(-3, 2, 130).view(130, 1)
    pair = E.split_pair(x, dtype)
    v = R.decode(pair, 7, 256)
    assert float(((v - x.double()).abs() - R.U_PAIR[dtype] * x.double().abs()).max()) <= 2.0 ** -25
    assert float((v.float() - E.join_pair(pair)).abs().max()) == 0.0
    mixed = R.encode_mixed(x, dtype)
    assert mixed.shape == (130, 512) and bool(torch.equal(mixed[:, :256], x.to(dtype)))
    vm = R.decode(mixed, 5, 256, out_lo8=1)
    assert float(((vm - x.double()).abs() - R.U_MIXED[dtype] * x.double().abs()).max()) <= 2.0 ** -24
    assert float((vm.float() - E.join_mixed(mixed)).abs().max()) == 0.0
    # a pitched copy decodes to the same values and keeps its padding
    wide = R.with_pitch(mixed, 512 + 64, 0x7e01)
    assert bool(torch.equal(R.decode(wide, 5, 256, out_lo8=1), vm)) and bool((wide[:, 512:].view(torch.int16) == 0x7e01).all())
    # the packed weight: 16-bit plane bit-exact, fp8 plane within e4m3's 2^-4 of the value
    W = (torch.randn(128, 256, generator=g) * 0.05).to(dtype)
    e8 = R.w8_exponent(W.float())
    Wp, w8 = R.pack_weight_mixed(W, e8)
    assert Wp.shape == (128, 384) and bool(torch.equal(Wp[:, :256], W)) and 128.0 <= float(W.float().abs().max()) * 2.0 ** e8 < 256.0
    assert float(((w8 - W.double()).abs() - 2.0 ** -4 * W.double().abs()).max()) <= 2.0 ** (-10 - e8)


def test_quickgelu_constants_are_four_times_the_fp32_host_error():
    """E_FN_GELU / E_FN_GELU_GRAD: the error of a plain fp32 evaluation against float64 on the inputs the GPU tests use (the pre-activations
    acc + bias of every shape and the saved pre-activation `aux`), times 4."""
    worst_g = worst_d = 0.0
    for route, fmt, K, dtype in [c + (d,) for c in CASES for d in R.DTYPES]:
        M, N, K = _shape(route, fmt, K)
        pr = R.Problem(fmt, dtype, min(M, 600), N, K)
        u = (pr.products()[0] + pr.bias.double())
        u32 = u.float()
        g32 = (u32 / (1.0 + torch.exp(-1.702 * u32))).double()
        g64 = R.quick_gelu(u32.double())
        worst_g = max(worst_g, float(((g32 - g64).abs() / g64.abs().clamp_min(1e-300)).max()))
        a = pr.aux.float()
        s = 1.0 / (1.0 + torch.exp(-1.702 * a))
        d32 = (s * (1.0 + 1.702 * a * (1.0 - s))).double()
        worst_d = max(worst_d, float(((d32 - R.quick_gelu_grad(a.double())).abs() / R.gelu_grad_envelope(a.double())).max()))
    print(f"fp32 host error: QuickGELU {worst_g:.3e} (relative), QuickGELU' {worst_d:.3e} (relative to G(u))")
    assert 4 * worst_g <= R.E_FN_GELU <= 4 * worst_g * 1.05
    assert 4 * worst_d <= R.E_FN_GELU_GRAD <= 4 * worst_d * 1.05
