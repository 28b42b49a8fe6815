"""Float64 references, seeded inputs and per-element error bounds of the stand-alone activation kernels (mvlpt_amd/csrc/activation.hip;
include/mvlpt_hip.h: mvlpt_op_activation_fwd / _bwd).  Plain torch; nothing here launches a kernel of the library.
tests/test_activation_ref.py checks the module without a GPU, tests/test_hip_activation.py uses it.

Reference.  The kernels read fp32 values (the pre-activation u, the gradient dA) and the saved 16-bit u, so the reference is the exact
function of those values in float64:
    GELU(u)  = u Phi(u)                Phi(u) = erfc(-u / sqrt 2) / 2        phi(u) = exp(-u^2 / 2) / sqrt(2 pi)
    GELU'(u) = Phi(u) + u phi(u)       G(u)   = Phi(u) + |u| phi(u)          (the envelope: the magnitude of the derivative's two terms;
                                                                              the derivative crosses zero near u = -0.75, so an error
                                                                              relative to it would be unbounded there)
Per-element bound, built as tests/gemm_ref.py builds its own: the value in front of the store is known to E_pre, and the store rounds it
once more to the output format,
    |got - ref| <= u_out (|ref| + E_pre) + floor + E_pre
with u_out / floor of gemm_ref.py (U_OUT16, U_PAIR, U_MIXED; the subnormal spacing of the format).  The inputs are exact, so
    forward   E_pre = E_FN |GELU(u)|
    backward  E_pre = E_FN' G(u) |dA| + 2^-24 |dA GELU'(u)|      (the second term: the fp32 product dA * GELU'(u) rounds once)
    saved u   E_pre = 0                                           (one 16-bit rounding of the fp32 input)
E_FN and E_FN' are the one part that is NOT derivable here: the device evaluates erfc and exp with its own fp32 library routines.  They
are 4x the largest error of a plain fp32 host evaluation of the same formula (torch float32, the erfc form) against float64, relative to
|GELU(u)| resp. G(u), over the inputs of the GPU tests (GRID, both 16-bit roundings of u for the backward) and over u in [-12, 12] in
steps of 2^-6.  The forward's error is largest on the negative tail, where it is the CONDITIONING of the formula, not the quality of the
routine: erfc(x) turns the 2^-24 rounding of its argument x = -u / sqrt 2 into 2 x^2 2^-24 of its result (u = -12: 8.6e-6), and the
device rounds that argument in the same way.  The backward's u is a 16-bit value, so u^2 / 2 is exact in fp32, and on the tail G(u) is
|u| phi(u), next to which Phi(u) and its error are smaller by u^2.
Measured: GELU 9.67e-6, GELU' 9.80e-7 -> the constants below; tests/test_activation_ref.py re-measures them and holds the constants to 4x.
"""
import math

import torch

from tests.gemm_ref import LO8_EXP, U_MIXED, U_OUT16, U_PAIR, decode_lo8, encode_mixed, violations, with_pitch      # noqa: F401

ACT_QUICKGELU, ACT_GELU = 0, 1                      # MVLPT_ACT_*
FORMATS = ["single", "pair", "mixed"]
FMT_CODE = {"single": 0, "pair": 1, "mixed": 2}     # MVLPT_ACT_OUT_*
DTYPES = [torch.float16, torch.bfloat16]
GRID = [(M, N) for M in (1, 77, 130) for N in (128, 256)]
FIXED_POINTS = [12.0, -12.0, 6.0, -6.0, 1.0, -1.0, 1e-3, -1e-3, 0.0, -0.0]

# 4x the measured fp32 host error (module docstring): relative to |GELU(u)| / to G(u)
E_FN_GELU = 3.87e-5
E_FN_GELU_GRAD = 3.93e-6

_SQRT1_2 = 0.7071067811865476
_INV_SQRT_2PI = 0.3989422804014327


# ------------------------------------------------------------------------------------------------ float64 functions
def Phi(u):
    return 0.5 * torch.erfc(-u * _SQRT1_2)


def phi(u):
    return _INV_SQRT_2PI * torch.exp(-0.5 * u * u)


def gelu(u):
    return u * Phi(u)


def gelu_grad(u):
    return Phi(u) + u * phi(u)


def gelu_grad_envelope(u):
    return Phi(u) + u.abs() * phi(u)


# ------------------------------------------------------------------------------------------------ plain fp32 evaluation (host)
def gelu_f32(u):
    """The kernel's formula in torch float32: u * (0.5 * erfc(-u / sqrt 2))."""
    u = u.float()
    return u * (0.5 * torch.erfc(-u * torch.tensor(_SQRT1_2, dtype=torch.float32)))


def gelu_grad_f32(u):
    u = u.float()
    c = torch.tensor(_INV_SQRT_2PI, dtype=torch.float32)
    return 0.5 * torch.erfc(-u * torch.tensor(_SQRT1_2, dtype=torch.float32)) + u * (c * torch.exp(-0.5 * (u * u)))


def ramp():
    """u in [-12, 12] in steps of 2^-6 (exact in fp32)."""
    return torch.arange(-12 * 64, 12 * 64 + 1, dtype=torch.float32) / 64.0


# ------------------------------------------------------------------------------------------------ inputs
def inputs(M, N):
    """(u, dA) fp32 [M, N]: u ~ N(0, 2) with FIXED_POINTS planted in columns 0-9 of every row, dA ~ N(0, 1) with an exact 0 in column 10
    and 2^-20 in column 11 of every row (the other columns put a random dA on every fixed point of u)."""
    g = torch.Generator().manual_seed(7919 * M + N)
    u = torch.randn(M, N, generator=g) * 2.0
    u[:, :len(FIXED_POINTS)] = torch.tensor(FIXED_POINTS)
    dA = torch.randn(M, N, generator=g)
    dA[:, 10] = 0.0
    dA[:, 11] = 2.0 ** -20
    return u, dA


# ------------------------------------------------------------------------------------------------ formats
def u_out(dtype, fmt):
    """(relative rounding, absolute floor) of a value stored in `fmt` (gemm_ref.u_out by format name)."""
    f16 = dtype == torch.float16
    if fmt == "single":
        return U_OUT16[dtype], (2.0 ** -25 if f16 else 0.0)
    if fmt == "mixed":
        return U_MIXED[dtype], (2.0 ** -25 if f16 else 2.0 ** -24)
    return U_PAIR[dtype], (2.0 ** -25 if f16 else 0.0)


def row_width(fmt, N):
    return N if fmt == "single" else 2 * N


def decode(out, fmt, N):
    """Float64 value of a kernel output [M, >= row_width] (the dense part is decoded; the pair planes are summed in float64)."""
    if fmt == "single":
        return out[:, :N].double()
    if fmt == "mixed":
        return out[:, :N].double() + decode_lo8(out[:, :2 * N], N)
    return out[:, :N].double() + out[:, N:2 * N].double()


def round_to_format(v, dtype, fmt):
    """fp32 -> the stored format and back, as float64 (what a kernel with an exact function would store)."""
    v = v.float()
    if fmt == "single":
        return v.to(dtype).double()
    if fmt == "mixed":
        p = encode_mixed(v, dtype)
        return p[:, :v.shape[1]].double() + decode_lo8(p, v.shape[1])
    hi = v.to(dtype)
    return hi.double() + (v - hi.float()).to(dtype).double()


# ------------------------------------------------------------------------------------------------ references and bounds
def _stored(ref, pre, dtype, fmt):
    ur, uf = u_out(dtype, fmt)
    return ref, ur * (ref.abs() + pre) + uf + pre


def fwd_reference(u, dtype, fmt):
    """{"out": (ref, bound), "u16": (ref, bound)} in float64 for the fp32 pre-activation u."""
    u = u.double()
    ref = gelu(u)
    ur, uf = u_out(dtype, "single")
    return {"out": _stored(ref, E_FN_GELU * ref.abs(), dtype, fmt), "u16": (u, ur * u.abs() + uf)}


def bwd_reference(dA, u16, dtype, fmt):
    """(ref, bound) in float64 for the fp32 gradient dA and the saved 16-bit pre-activation u16."""
    dA, u = dA.double(), u16.double()
    ref = dA * gelu_grad(u)
    return _stored(ref, E_FN_GELU_GRAD * gelu_grad_envelope(u) * dA.abs() + 2.0 ** -24 * ref.abs(), dtype, fmt)


def measure_fn_error():
    """(worst GELU error relative to |GELU|, worst GELU' error relative to G) of the fp32 host evaluation over GRID and the ramp."""
    us = [ramp()] + [inputs(M, N)[0].reshape(-1) for M, N in GRID]
    worst_g = worst_d = 0.0
    for u in us:
        r = gelu(u.double())
        e = (gelu_f32(u).double() - r).abs()
        assert bool((e[r == 0] == 0).all())           # u = +-0: exact
        worst_g = max(worst_g, float((e / r.abs().clamp_min(1e-300))[r != 0].max()))
        for a in [u] + [u.to(d).float() for d in DTYPES]:      # the backward reads the 16-bit saved u
            d = (gelu_grad_f32(a).double() - gelu_grad(a.double())).abs() / gelu_grad_envelope(a.double())
            worst_d = max(worst_d, float(d.max()))
    return worst_g, worst_d


assert math.isclose(_SQRT1_2, math.sqrt(0.5)) and math.isclose(_INV_SQRT_2PI, 1.0 / math.sqrt(2.0 * math.pi))
