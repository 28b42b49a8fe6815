"""Float64 restatement, seeded inputs and per-element error bounds of the wide-head attention forward (mvlpt_amd/csrc/attention_wide.hip;
include/mvlpt_hip.h: mvlpt_op_attention_wide_fwd).  Plain torch; nothing here launches a kernel of the library.
tests/test_attention_wide_ref.py checks the module without a GPU, tests/test_hip_attention_wide.py uses it.

Reference.  The kernel reads 16-bit q, k, v, so the reference is the exact function of those values in float64, per (sequence, head):
    s_j = q . k_j / sqrt(w)     p_j = exp(s_j - M), M = max_j s_j     l = sum_j p_j     O_c = sum_j p_j v_jc / l     lse = M + ln l

Bound (a formula of float64 magnitudes, nothing measured).  u16 = 2^-11 (fp16) / 2^-8 (bf16) is the rounding of the 16-bit type, u32 = 2^-23
one fp32 operation (twice the rounding unit: the matrix unit's accumulation may truncate).  The device differs from the reference by
  1. the score.  Products of two 16-bit values are exact in fp32; their sum over w terms, the scale (1/sqrt(w) * log2 e, one rounded fp32
     constant) and the FMA that subtracts the running maximum leave, in natural-log units and with A_j = sum_i |q_i k_ji| / sqrt(w),
         d_j = u32 ((w + 1) A_j + 2 |s_j| + max_k |s_k|).
     The running maximum itself drops out: the softmax does not depend on the shift, the rescaling by alpha multiplies the sum and the
     accumulator by the same number, and only those multiplications round (n_chunks u32, counted below).
  2. the exponential: p_j is known to rho_j = d_j + 2^-22 (v_exp_f32: one ulp), relative.
  3. the rounding of P to 16 bit: u16 p_j, and for fp16 a p_j below the smallest normal (2^-14; 2^-13 here, p_j being known to rho_j only)
     may be lost entirely (subnormal operands of the matrix unit): the whole p_j counts.  eta_j = u16 + [fp16 and p_j < 2^-13].
  4. the fp32 accumulation of P V over L terms and n_chunks rescalings: (L + n_chunks) u32 sum_j p_j |v_jc|;
     of the row sum: (L + n_chunks) u32 l.
  5. 1 / l and its product with the accumulator: 3 u32 |O_c|.
  6. the output rounding: u16 |O_c| + 2^-25 (fp16: half the subnormal spacing; bf16: 0).
To first order, with B_c = sum_j p_j |v_jc| / l and R = sum_j rho_j p_j / l, Rv_c = sum_j (rho_j + eta_j) p_j |v_jc| / l:
    |O~_c - O_c| <= 1.01 [ Rv_c + (L + n_chunks) u32 B_c + |O_c| (R + (L + n_chunks) u32 + 3 u32) ] + u16 |O_c| (1 + e) + floor
(1.01: the products of two of these terms; every one is below 1e-2.  e: the first bracket relative to |O_c|, i.e. the value that is rounded
is ref + error.)  The lse sees the score error of the maximum, the weighted score error of the sum, the sum's accumulation, log2 (one ulp
of its result) and three fp32 operations on values of size |M|, |ln l| and |lse|:
    |lse~ - lse| <= 1.01 [ max_j d_j + R + (L + n_chunks) u32 ] + 4 u32 (|M| + |ln l| + |lse|)

Inputs.  q, k ~ N(0, 1.5^2), v ~ N(0, 1), rounded to the 16-bit type: scores have a spread of 2.25, so the softmax is peaked (a handful of
keys carry most of a row's weight) and every wrong reference of tests/test_attention_wide_ref.py — scale 1/8, head columns 64.. dropped,
the clamped key L counted, the neighbouring head's V — moves some element by far more than the bound.
"""
import math

import torch

from tests.gemm_ref import U_OUT16, violations      # noqa: F401

WIDTHS = (80, 96, 112, 128)
U32 = 2.0 ** -23
CHUNK = 64          # keys per streamed chunk (attention_wide.hip WCK)
F16, BF16 = torch.float16, torch.bfloat16

# (w, L, H, N, q_rows, want_lse, dtype): every width; L = 1, below one tile, one chunk, one key into the second chunk, two chunks and a
# bit, ViT-H/14's 257 (one key into the fifth); one and three heads; one and two sequences; every query and the CLS query only
CASES = [
    (80, 1, 1, 1, 0, True, F16), (80, 15, 3, 2, 0, True, F16), (80, 64, 1, 2, 0, False, BF16), (80, 65, 3, 1, 0, True, F16),
    (80, 130, 1, 2, 1, True, BF16), (80, 257, 3, 2, 0, True, F16), (80, 257, 3, 2, 1, False, BF16),
    (96, 15, 1, 1, 1, True, BF16), (96, 65, 3, 2, 0, True, F16), (96, 257, 1, 1, 0, False, F16),
    (112, 1, 3, 2, 0, True, BF16), (112, 64, 3, 1, 1, True, F16), (112, 130, 1, 2, 0, True, F16), (112, 257, 3, 1, 0, True, BF16),
    (128, 15, 3, 2, 0, False, F16), (128, 65, 1, 1, 0, True, BF16), (128, 130, 3, 2, 1, True, F16), (128, 257, 1, 2, 0, True, BF16),
]


def case_id(c):
    w, L, H, N, q_rows, want_lse, dtype = c
    return f"w{w}-L{L}-H{H}-N{N}-q{q_rows}-{'lse' if want_lse else 'nolse'}-{'f16' if dtype == F16 else 'bf16'}"


def inputs(w, L, H, N, dtype):
    """qkv [N*L, 3*H*w] in `dtype` on the host.  Sequence n is drawn from its own generator (seeded by w, L, H, n): sequence 0 of an
    N = 1 problem is sequence 0 of the N = 2 problem."""
    d = H * w
    rows = []
    for n in range(N):
        g = torch.Generator().manual_seed(1000003 * w + 7919 * L + 31 * H + n)
        t = torch.randn(L, 3 * d, generator=g)
        t[:, :2 * d] *= 1.5
        rows.append(t)
    return torch.cat(rows).to(dtype)


def split_heads(qkv, N, L, H, w):
    """(q, k, v) float64 [N, H, L, w] of qkv [N*L, 3*H*w]."""
    x = qkv.double().view(N, L, 3, H, w).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def reference(qkv, N, L, H, w, mutant=None):
    """(out [N*L, H*w], lse [N*H*L]) in float64.  mutant: one of the deliberately wrong references of tests/test_attention_wide_ref.py
    ("scale8", "cols64", "key_L", "next_head_v")."""
    q, k, v = split_heads(qkv, N, L, H, w)
    if mutant == "cols64":
        q, k = q[..., :64], k[..., :64]
    if mutant == "key_L":                                   # the clamped duplicate of key L - 1 takes part
        k, v = torch.cat([k, k[:, :, -1:]], 2), torch.cat([v, v[:, :, -1:]], 2)
    if mutant == "next_head_v":
        v = v.roll(-1, 1)
    s = q @ k.transpose(-1, -2) * (0.125 if mutant == "scale8" else 1.0 / math.sqrt(w))
    lse = torch.logsumexp(s, -1)
    out = torch.softmax(s, -1) @ v
    return out.permute(0, 2, 1, 3).reshape(N * L, H * w), lse.reshape(N * H * L)


def reference_and_bound(qkv, N, L, H, w):
    """{"out": (ref, bound) [N*L, H*w], "lse": (ref, bound) [N*H*L]} in float64 (module docstring)."""
    dtype = qkv.dtype
    u16 = U_OUT16[dtype]
    f16 = dtype == F16
    nacc = (L + (L + CHUNK - 1) // CHUNK) * U32
    q, k, v = split_heads(qkv, N, L, H, w)
    isw = 1.0 / math.sqrt(w)
    s = q @ k.transpose(-1, -2) * isw                       # [N, H, L, L]
    A = q.abs() @ k.abs().transpose(-1, -2) * isw
    M = s.max(-1, keepdim=True).values
    p = (s - M).exp()
    l = p.sum(-1, keepdim=True)
    dj = U32 * ((w + 1) * A + 2 * s.abs() + s.abs().max(-1, keepdim=True).values)
    rho = dj + 2.0 ** -22
    eta = torch.full_like(p, u16) + ((p < 2.0 ** -13).double() if f16 else 0.0)
    O = p @ v / l
    B = p @ v.abs() / l
    R = (rho * p).sum(-1, keepdim=True) / l
    Rv = ((rho + eta) * p) @ v.abs() / l
    pre = 1.01 * (Rv + nacc * B + O.abs() * (R + nacc + 3 * U32))
    b_out = pre + u16 * (O.abs() + pre) + (2.0 ** -25 if f16 else 0.0)
    lse = M + l.log()
    b_lse = 1.01 * (dj.max(-1, keepdim=True).values + R + nacc) + 4 * U32 * (M.abs() + l.log().abs() + lse.abs())
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(N * L, H * w)
    return {"out": (flat(O), flat(b_out)), "lse": (lse.reshape(N * H * L), b_lse.reshape(N * H * L))}


def computed_rows(N, L, q_rows):
    """Mask [N*L] of the token rows the kernel writes."""
    r = torch.arange(N * L) % L
    return r < (min(q_rows, L) if q_rows > 0 else L)


def computed_lse(N, L, H, q_rows):
    r = torch.arange(N * H * L) % L
    return r < (min(q_rows, L) if q_rows > 0 else L)
