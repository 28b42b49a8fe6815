"""Float64 references, seeded inputs and per-element error bounds of the MFMA GEMMs (mvlpt_amd/csrc/gemm.hip) for every epilogue 0-7
and every A-operand format (single 16-bit, hi|lo pair, mixed pair).  Plain torch on whatever device the tensors live on; nothing here
launches a kernel of the library.  tests/test_gemm_ref.py checks the module without a GPU, tests/test_hip_gemm_matrix.py uses it.

Reference.  The operands are the 16-bit (and fp8) values the kernel reads, so the reference is the exact product of those values in
float64 and only the kernel's own arithmetic differs:
    single  acc = A16 Bt16^T
    pair    acc = (A_hi + A_lo) Bt16^T
    mixed   acc = A_hi W16^T + (A_lo8 2^-LO8_EXP) (W8 2^-w8_exp)^T          (e5m2 residual bytes x the weight's e4m3 copy)
QuickGELU(u) = u s(u) and QuickGELU'(u) = s (1 + 1.702 u (1 - s)), s = sigmoid(1.702 u), are evaluated in float64.

Per-element bound (derived; it holds for any accumulation order).  With n = K_eff products per output element (K single, 2K pair and
mixed pair), fp32 accumulation of the exact 16-bit / fp8 products loses at most (n - 1) 2^-24 S, S = |A| |Bt|^T (a second float64 matmul);
the bias and the residual add two more roundings of at most 2^-24 (S + |bias| + |resid|) each:
    E_acc = (K_eff + 2) 2^-24 (S + |bias| + |resid|)
and the stored value is rounded once more to the output format:
    |got - ref| <= u_out (|ref| + E_pre) + floor + E_pre
u_out: 2^-11 (fp16), 2^-8 (bf16), 2^-24 (fp32), 2^-22 / 2^-16 (fp16 / bf16 hi|lo pair: kernels.h "to ~22 bits", SPLIT_TOL "22 / 16
significant bits"), 2^-14 / 2^-11 (mixed pair, kernels.h).  floor: the spacing of the format's subnormals, where the relative bound cannot
hold: 2^-25 for every fp16 output (fp16 subnormals are 2^-24 apart; the pair's lo plane is the one that gets there), 2^-24 for a bf16 mixed
pair (e5m2 subnormals are 2^-16 apart and the byte is scaled by 2^7), 0 otherwise.
E_pre is E_acc for epilogues 0 / 2 / 4 / 7 and the saved pre-activation.  QuickGELU (1 / 5): u = acc + bias carries E_acc and |QuickGELU'|
<= 1.1, so E_pre = 1.1 E_acc + E_fn |QuickGELU(u)|.  QuickGELU' (3 / 6): E_pre = |g'(u)| E_acc + E_fn G(u) |acc|, with G(u) = s + 1.702 |u| s (1 - s)
the magnitude of the factor's two terms (the factor itself crosses zero, an error relative to it would be unbounded there).
E_fn is the one term that is NOT derivable here: the device evaluates s with its approximate exp2 and reciprocal.  It is 4x the largest
error of a plain fp32 host evaluation of the same formula against float64 on the test's own inputs (two roughly 1-ulp hardware
approximations in series), relative to |QuickGELU(u)| resp. G(u).  Measured over every shape of the matrix (DESIGN.md "GEMM kernel tests"):
QuickGELU 6.82e-7, QuickGELU' 9.96e-7 (the 1 - s of large positive u) -> the constants below; tests/test_gemm_ref.py re-measures them and holds the constants to 4x.
"""
import functools

import torch

EPI_STORE16, EPI_GELU, EPI_RESID32, EPI_GELUBWD, EPI_STORE32, EPI_GELU_SPLIT, EPI_GELUBWD_SPLIT, EPI_STORE_SPLIT = range(8)
FORMATS = ["single", "pair", "mixed"]
A_SPLIT = {"single": 0, "pair": 1, "mixed": 2}
DTYPES = [torch.float16, torch.bfloat16]
# every epilogue the launchers accept per operand format (gemm.hip launch_geo / launch_pc / launch_pcp)
LEGAL_EPIS = {"single": list(range(8)), "pair": list(range(8)),
              "mixed": [EPI_RESID32, EPI_STORE32, EPI_GELU_SPLIT, EPI_GELUBWD_SPLIT, EPI_STORE_SPLIT]}
K_VALUES = {"single": [64, 128, 192, 768], "pair": [64, 128, 192, 768], "mixed": [128, 256, 384, 768]}
LO8_EXP = {torch.float16: 10, torch.bfloat16: 7}

# Routes of the matrix on a 32-CU partition stream: name -> (M ragged, M an exact multiple of the tile, M = tiles + one row, N, tile_m).
# The three M values have the same tile counts, so they take the same kernel.
ROUTES32 = {
    "pcp": (1400, 1536, 1281, 1152, 256),            # 54 tiles of 256x128 (1.7 rounds); N % 256 != 0 keeps it off 256x256
    "big_multi": (2700, 2816, 2561, 3072, 256),      # 132 tiles of 256x256: 4.1 rounds
    "big_one": (1900, 2048, 1793, 1024, 256),        # 32 tiles of 256x256: exactly one round
    "small": (1100, 1152, 1025, 1024, 128),          # 72 tiles of 128x128, two per compute unit: 1.1 rounds
    "pc": (391, 512, 385, 512, 128),                 # 16 tiles of 128x128, pair / mixed operands only
}
PHASED32 = {"single": (1400, 1152, 2048), "pair": (1400, 1152, 1024)}      # K_eff = 2048: the long-K kernel (no mixed pair)

U_OUT16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
U_PAIR = {torch.float16: 2.0 ** -22, torch.bfloat16: 2.0 ** -16}
U_MIXED = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -11}
GELU_SLOPE_MAX = 1.1            # sup |QuickGELU'| = 1.0998 (at 1.702 u = 2.40)
# 4x the measured fp32 host error (module docstring): relative to |QuickGELU(u)| / to G(u)
E_FN_GELU = 2.73e-6
E_FN_GELU_GRAD = 3.99e-6

# the project's existing max-norm bounds (tests/test_hip_ops.py TOL, 2e-5, SPLIT_TOL, 2e-6 {1, 40}; tests/test_hip_mixed_pair.py)
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
SPLIT_TOL = {torch.float16: 3e-6, torch.bfloat16: 6e-5}
MIXED_GEMM_TOL = {torch.float16: 4e-5, torch.bfloat16: 4e-4}
MIXED_PAIR_TOL = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -11}


def maxnorm_tol(fmt, dtype, epi, which="out"):
    if which == "out2" or epi in (EPI_STORE16, EPI_GELU, EPI_GELUBWD):
        return TOL[dtype]
    if fmt == "single":
        # a single operand with a pair output: the product is fp32-accurate, the pair carries it
        return 2e-5
    if fmt == "pair":
        return SPLIT_TOL[dtype] if epi in (EPI_RESID32, EPI_STORE32, EPI_STORE_SPLIT) else 2e-6 * (1 if dtype == torch.float16 else 40)
    return MIXED_GEMM_TOL[dtype] if epi in (EPI_RESID32, EPI_STORE32, EPI_STORE_SPLIT) else 2 * MIXED_PAIR_TOL[dtype]


def relerr(a, b):
    return float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-30)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=2)
def _master(M, N, K):
    g = torch.Generator().manual_seed(100003 * M + 101 * N + K)
    return dict(A=torch.randn(M, K, generator=g), W=torch.randn(N, K, generator=g) * K ** -0.5, bias=torch.randn(N, generator=g),
                resid=torch.randn(M, N, generator=g), aux=torch.randn(M, N, generator=g) * 2.0)


def w8_exponent(W):
    """The exponent op_pack_weight_mixed gives a weight: 128 <= max|W| 2^e < 256."""
    import math
    return 7 - math.floor(math.log2(float(W.abs().max())))


def encode_mixed(x, dtype, pitch=None, fill=0):
    """fp32 [M, d] -> mixed pair rows [M, pitch >= 2d] of `dtype`: [hi | e5m2((x - hi) 2^LO8_EXP) bytes | unused]; every 16-bit slot
    that is not part of the value holds the bit pattern `fill`."""
    M, d = x.shape
    pitch = pitch or 2 * d
    hi = x.to(dtype)
    lo = ((x - hi.float()) * 2.0 ** LO8_EXP[dtype]).clamp(-57344.0, 57344.0).to(torch.float8_e5m2)
    out = torch.full((M, pitch), fill, dtype=torch.int16)
    out[:, :d] = hi.view(torch.int16)
    out[:, d:d + d // 2] = lo.view(torch.uint8).contiguous().view(torch.int16)
    return out.view(dtype)


def decode_lo8(p, d):
    """The residual plane of mixed-pair rows [M, >= 2d], as float64 values."""
    b = p[:, d:d + d // 2].contiguous().view(torch.uint8).view(torch.float8_e5m2)
    return b.to(torch.float32).double() * 2.0 ** -LO8_EXP[p.dtype]


def pack_weight_mixed(W16, e8):
    """W16 [N, K] (16-bit values) -> [N, 3K/2] = [W16 | e4m3(W 2^e8) bytes] and the float64 value of the fp8 plane."""
    w8 = (W16.float() * 2.0 ** e8).to(torch.float8_e4m3fn)
    packed = torch.cat([W16.view(torch.int16), w8.view(torch.uint8).contiguous().view(torch.int16)], dim=1).view(W16.dtype)
    return packed.contiguous(), w8.to(torch.float32).double() * 2.0 ** -e8


def with_pitch(t, pitch, fill):
    """Rows of `t` at a pitch of `pitch` 16-bit elements; the padding holds the 16-bit pattern `fill`."""
    out = torch.full((t.shape[0], pitch), fill, dtype=torch.int16, device=t.device)
    out[:, :t.shape[1]] = t.view(torch.int16)
    return out.view(t.dtype)


class Problem:
    """Seeded operands of one GEMM in the format the kernel reads (host tensors) and the float64 parts of its exact product."""

    def __init__(self, fmt, dtype, M, N, K, m_alloc=None):
        m = _master(m_alloc or M, N, K)
        self.fmt, self.dtype, self.M, self.N, self.K = fmt, dtype, M, N, K
        A = m["A"][:M]
        W16 = m["W"].to(dtype)
        self.bias, self.resid, self.aux = m["bias"], m["resid"][:M].contiguous(), m["aux"][:M].to(dtype).contiguous()
        self.w8_exp, self.ldb = 0, 0
        if fmt == "single":
            self.A = A.to(dtype).contiguous()
            self.Bt = W16.contiguous()
            self.parts = [(self.A, W16)]
        elif fmt == "pair":
            hi = A.to(dtype)
            lo = (A - hi.float()).to(dtype)
            self.A = torch.cat([hi, lo], dim=1).contiguous()
            self.Bt = W16.contiguous()
            self.parts = [(hi, W16), (lo, W16)]
        else:
            self.A = encode_mixed(A, dtype)
            self.w8_exp = w8_exponent(W16.float())
            self.Bt, w8 = pack_weight_mixed(W16, self.w8_exp)
            self.ldb = self.Bt.shape[1]
            self.parts = [(self.A[:, :K], W16), (decode_lo8(self.A, K), w8)]
        self.k_eff = K if fmt == "single" else 2 * K

    def products(self, device="cpu", rows=None):
        """(acc, S) = (sum of the exact products, sum of their magnitudes) in float64 on `device`, for all rows or a slice of them."""
        acc = S = None
        for a, b in self.parts:
            a = (a if rows is None else a[rows]).to(device).double()
            b = b.to(device).double()
            p, q = a @ b.t(), a.abs() @ b.abs().t()
            acc, S = (p, q) if acc is None else (acc + p, S + q)
        return acc, S


# ------------------------------------------------------------------------------------------------ references and bounds
def sigmoid1702(u):
    return 1.0 / (1.0 + torch.exp(-1.702 * u))


def quick_gelu(u):
    return u * sigmoid1702(u)


def quick_gelu_grad(u):
    s = sigmoid1702(u)
    return s * (1.0 + 1.702 * u * (1.0 - s))


def gelu_grad_envelope(u):
    s = sigmoid1702(u)
    return s + 1.702 * u.abs() * s * (1.0 - s)


def u_out(dtype, epi, out_lo8, which="out"):
    """(relative rounding, absolute floor) of the stored value."""
    f16 = dtype == torch.float16
    if which == "out2" or epi in (EPI_STORE16, EPI_GELU, EPI_GELUBWD):
        return U_OUT16[dtype], (2.0 ** -25 if f16 else 0.0)
    if epi in (EPI_RESID32, EPI_STORE32):
        return 2.0 ** -24, 0.0
    if out_lo8 and epi != EPI_STORE_SPLIT:
        return U_MIXED[dtype], (2.0 ** -25 if f16 else 2.0 ** -24)
    return U_PAIR[dtype], (2.0 ** -25 if f16 else 0.0)


def reference(epi, acc, S, k_eff, dtype, bias=None, resid=None, aux=None, out_lo8=0):
    """{"out": (ref, bound)[, "out2": (ref, bound)]} in float64 from the exact product `acc`, its magnitude sum `S` and the epilogue
    operands (aux: the 16-bit pre-activation)."""
    zero = torch.zeros((), dtype=torch.float64, device=acc.device)
    b = bias.double().to(acc.device) if bias is not None else zero
    r = resid.double().to(acc.device) if (resid is not None and epi == EPI_RESID32) else zero
    e_acc = (k_eff + 2) * 2.0 ** -24 * (S + b.abs() + r.abs())
    return finish(epi, acc + b + r, e_acc, dtype, aux=aux, out_lo8=out_lo8)


def finish(epi, v, e_v, dtype, aux=None, out_lo8=0):
    """The non-linear part of the epilogue and the output rounding on the linear value v (float64) that the kernel knows to e_v."""
    res = {}
    if epi in (EPI_STORE16, EPI_STORE32, EPI_STORE_SPLIT, EPI_RESID32):
        ref, pre = v, e_v
    elif epi in (EPI_GELU, EPI_GELU_SPLIT):
        ref = quick_gelu(v)
        pre = GELU_SLOPE_MAX * e_v + E_FN_GELU * ref.abs()
        ur, uf = u_out(dtype, epi, out_lo8, "out2")
        res["out2"] = (v, ur * (v.abs() + e_v) + uf + e_v)
    else:
        a = aux.double().to(v.device)
        g = quick_gelu_grad(a)
        ref = v * g
        pre = g.abs() * e_v + E_FN_GELU_GRAD * gelu_grad_envelope(a) * v.abs()
    ur, uf = u_out(dtype, epi, out_lo8)
    res["out"] = (ref, ur * (ref.abs() + pre) + uf + pre)
    return res


FOLD_LN_EPS = 1e-5


def folded_linear(acc, S, k_eff, K, part, nt, colsum, bias2):
    """(v, e_v) of a folded consumer (kernels.h "LayerNorm folding"): v = a acc + cc colsum + bias2 with, per row, mean = s1 / K,
    var = max(s2 / K - mean^2, 0), a = (var + eps)^-1/2, cc = -a mean, {s1, s2} the sums of the row's first `nt` partials.
    Error (fp32, any order): the two sums lose (nt - 1) 2^-24 of themselves, so var + eps is known to (nt + 3) 2^-24 (s2 / K + mean^2),
    i.e. to kappa (nt + 3) 2^-24 of itself with kappa = (s2 / K + mean^2) / (var + eps) (the cancellation of a row with a large mean);
    the inverse square root halves that and adds its own approximation (4 x 2^-24: an approximate instruction, as for the QuickGELU
    factor); cc adds the mean's (nt + 1) 2^-24; the two fused multiply-adds round twice."""
    u = 2.0 ** -24
    p = part.double()[:, :nt]
    s1, s2 = p[..., 0].sum(1), p[..., 1].sum(1)
    mean = s1 / K
    m2 = s2 / K
    var = (m2 - mean * mean).clamp_min(0.0)
    a = (var + FOLD_LN_EPS).rsqrt()
    cc = -a * mean
    kappa = (m2 + mean * mean) / (var + FOLD_LN_EPS)
    eps_a = u * (0.5 * kappa * (nt + 3) + 4)
    eps_cc = eps_a + u * (nt + 1)
    a, cc, eps_a, eps_cc = (t.view(-1, 1) for t in (a, cc, eps_a, eps_cc))
    cs, b2 = colsum.double().view(1, -1), bias2.double().view(1, -1)
    v = a * acc + cc * cs + b2
    e_acc = (k_eff + 2) * u * S
    e_v = a * e_acc + eps_a * (a * acc).abs() + eps_cc * (cc * cs).abs() + 2 * u * ((a * acc).abs() + (cc * cs).abs() + b2.abs())
    return v, e_v


def decode(out, epi, N, out_lo8=0):
    """Float64 value of a kernel output: 16-bit / fp32 [M, N], hi|lo pair or mixed pair [M, >= 2N] (the dense part is decoded).
    The pair decoders are join_pair / join_mixed of mvlpt_amd/engine.py with the sum taken in float64 (their fp32 sum rounds away the
    end of a lo plane that sits far below its hi); tests/test_gemm_ref.py holds them to those two."""
    if epi in (EPI_GELU_SPLIT, EPI_GELUBWD_SPLIT, EPI_STORE_SPLIT):
        p = out[:, :2 * N]
        if out_lo8 and epi != EPI_STORE_SPLIT:
            return p[:, :N].double() + decode_lo8(p, N)
        return p[:, :N].double() + p[:, N:].double()
    return out.double()


def violations(got, ref, bound):
    """(number of elements outside the bound, largest |got - ref| / bound); a NaN counts as outside."""
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    return int(bad.sum()), ratio


# ------------------------------------------------------------------------------------------------ plain fp32 evaluation (host)
def fp32_host(problem, epi, out_lo8=0, with_out2=True):
    """The same GEMM and epilogue in plain fp32 torch on the host, rounded to the output format: {"out": float64[, "out2": float64]}."""
    dtype, N = problem.dtype, problem.N
    acc = None
    for a, b in problem.parts:
        p = a.float() @ b.float().t()
        acc = p if acc is None else acc + p
    bias = problem.bias
    res = {}
    if epi in (EPI_STORE16, EPI_STORE32, EPI_STORE_SPLIT):
        v = acc + bias
    elif epi == EPI_RESID32:
        v = acc + bias + problem.resid
    elif epi in (EPI_GELU, EPI_GELU_SPLIT):
        u = acc + bias
        v = u / (1.0 + torch.exp(-1.702 * u))
        res["out2"] = u.to(dtype).double()
    else:
        a = problem.aux.float()
        s = 1.0 / (1.0 + torch.exp(-1.702 * a))
        v = acc * (s * (1.0 + 1.702 * a * (1.0 - s)))
    res["out"] = round_to_format(v, dtype, epi, out_lo8)
    return res


def round_to_format(v, dtype, epi, out_lo8=0):
    """fp32 -> the stored format and back, as float64."""
    if epi in (EPI_RESID32, EPI_STORE32):
        return v.double()
    if epi in (EPI_STORE16, EPI_GELU, EPI_GELUBWD):
        return v.to(dtype).double()
    if out_lo8 and epi != EPI_STORE_SPLIT:
        p = encode_mixed(v, dtype)
        return p[:, :v.shape[1]].double() + decode_lo8(p, v.shape[1])
    hi = v.to(dtype)
    return hi.double() + (v - hi.float()).to(dtype).double()
