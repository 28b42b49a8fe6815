"""The activation references, decoders and bounds of tests/activation_ref.py, checked without a GPU: the float64 reference rounded to
each output format and a plain fp32 host evaluation stay inside every per-element bound at every point of the GPU tests' grid, a
perturbed element and the `1 + erf` form on the negative tail fall outside, and the two measured constants are re-measured."""
import pytest
import torch

from tests import activation_ref as R


def test_float64_functions():
    u = torch.linspace(-12, 12, 4801, dtype=torch.float64)
    assert float((R.gelu(u) - torch.nn.functional.gelu(u)).abs().max()) < 4e-15      # (absolute: torch's own form cancels on the tail)
    v = u.clone().requires_grad_(True)
    torch.nn.functional.gelu(v).sum().backward()
    assert float((R.gelu_grad(u) - v.grad).abs().max()) < 4e-15
    assert bool((R.gelu_grad_envelope(u) >= R.gelu_grad(u).abs()).all())
    # the erfc form keeps the tail: Phi(-12) = 1.776e-33 to every digit float64 has
    assert abs(float(R.Phi(torch.tensor(-12.0, dtype=torch.float64))) / 1.7764821120776768e-33 - 1.0) < 1e-12


def test_inputs_carry_the_planted_points():
    for M, N in R.GRID:
        u, dA = R.inputs(M, N)
        assert u.shape == dA.shape == (M, N)
        assert bool((u[:, :10] == torch.tensor(R.FIXED_POINTS)).all()) and bool(torch.signbit(u[:, 9]).all())
        assert bool((dA[:, 10] == 0).all()) and bool((dA[:, 11] == 2.0 ** -20).all())
        assert float(u.abs().max()) <= 12.0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("M,N", R.GRID)
def test_reference_and_fp32_host_are_inside_every_bound(M, N, fmt, dtype):
    u, dA = R.inputs(M, N)
    fwd = R.fwd_reference(u, dtype, fmt)
    ref, b = fwd["out"]
    assert bool(torch.isfinite(b).all()) and bool((b >= 0).all())      # a bound at every grid point (u = +-0 in bf16: 0, the exact 0 is asked for)
    # the float64 reference itself, stored in the format, and the fp32 host evaluation of the kernel's formula
    for got in (R.round_to_format(ref, dtype, fmt), R.round_to_format(R.gelu_f32(u), dtype, fmt)):
        assert R.violations(got, ref, b)[0] == 0
    ur, ub = fwd["u16"]
    assert R.violations(u.to(dtype).double(), ur, ub)[0] == 0
    u16 = u.to(dtype)
    ref, b = R.bwd_reference(dA, u16, dtype, fmt)
    for got in (R.round_to_format(ref, dtype, fmt), R.round_to_format(dA * R.gelu_grad_f32(u16), dtype, fmt)):
        assert R.violations(got, ref, b)[0] == 0
    # dA = 0 gives exactly 0, and nothing but 0 passes there in a format without a floor
    assert bool((ref[:, 10] == 0).all())
    # one element moved by four times its bound is caught, wherever it sits (the smallest-magnitude element included)
    good = R.round_to_format(ref, dtype, fmt)
    idx = int(ref.abs().argmin())
    p = good.clone().view(-1)
    p[idx] = ref.view(-1)[idx] + 4 * b.reshape(-1)[idx] + 1e-300
    assert R.violations(p.view_as(good), ref, b)[0] == 1


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
def test_bound_catches_the_cancelling_form_on_the_negative_tail(dtype):
    """0.5 u (1 + erf(u / sqrt 2)) in fp32 loses its bits below u = -2 (at u = -6 it is 0, the true value -5.9e-9) and QuickGELU is
    another function altogether: the first hides under a max-norm, both fall outside the per-element bound of the pair format."""
    u, _ = R.inputs(77, 128)
    ref, b = R.fwd_reference(u, dtype, "pair")["out"]
    uf = u.float()
    erf_form = 0.5 * uf * (1.0 + torch.erf(uf * 0.7071067811865476))
    got = R.round_to_format(erf_form, dtype, "pair")
    assert float((got - ref).abs().max()) / float(ref.abs().max()) < 1e-4          # invisible to a max-norm
    bad = ~((got - ref).abs() <= b)
    assert int(bad[u < -2].sum()) > 100 and int(bad[u > -1].sum()) == 0            # the tail, and only the tail
    if dtype == torch.bfloat16:                                                    # (fp16 cannot hold 5.9e-9: its floor covers u = -6)
        assert bool(bad[:, 3].all())
    quick = R.round_to_format(uf * torch.sigmoid(1.702 * uf), dtype, "pair")
    assert R.violations(quick, ref, b)[0] > 0.5 * u.numel()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["fp16", "bf16"])
def test_decoders_round_trip(dtype):
    from mvlpt_amd import engine as E
    x, _ = R.inputs(130, 256)
    pair = E.split_pair(x, dtype)
    assert bool(torch.equal(R.decode(pair, "pair", 256), R.round_to_format(x, dtype, "pair")))
    assert float((R.decode(pair, "pair", 256).float() - E.join_pair(pair)).abs().max()) == 0.0
    mixed = R.encode_mixed(x, dtype)
    assert bool(torch.equal(R.decode(mixed, "mixed", 256), R.round_to_format(x, dtype, "mixed")))
    assert float((R.decode(mixed, "mixed", 256).float() - E.join_mixed(mixed)).abs().max()) == 0.0
    wide = R.with_pitch(mixed, 512 + 8, 0x7e01)
    assert bool(torch.equal(R.decode(wide, "mixed", 256), R.decode(mixed, "mixed", 256)))
    assert bool(torch.equal(R.decode(x.to(dtype), "single", 256), x.to(dtype).double()))
    for fmt in R.FORMATS:
        ur, uf = R.u_out(dtype, fmt)
        assert float(((R.round_to_format(x, dtype, fmt) - x.double()).abs() - ur * x.double().abs()).max()) <= uf


def test_gelu_constants_are_four_times_the_fp32_host_error():
    """E_FN_GELU / E_FN_GELU_GRAD: the error of a plain fp32 evaluation (erfc form) against float64 over the GPU tests' inputs and over
    u in [-12, 12] in steps of 2^-6, times 4."""
    worst_g, worst_d = R.measure_fn_error()
    print(f"fp32 host error: GELU {worst_g:.3e} (relative), GELU' {worst_d:.3e} (relative to G(u))")
    assert 4 * worst_g <= R.E_FN_GELU <= 4 * worst_g * 1.05
    assert 4 * worst_d <= R.E_FN_GELU_GRAD <= 4 * worst_d * 1.05
