"""Plain float64 references of the dense head, the loss and the fp32 glue, and the seeded inputs the GPU tests draw
(tests/test_hip_head.py, tests/test_hip_glue.py).  Nothing here touches the device: tests/test_head_ref.py pins every reference to
torch autograd in float64 or to oracle/clip_oracle.py, and derives the bounds that are not the project's own, on a machine without a GPU."""
import math

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ shapes of the issue
HEAD_EMBED = [64, 128, 512, 576, 768, 1024]
HEAD_BC = [(1, 1), (3, 2), (5, 7), (17, 255), (64, 257), (256, 1000), (13, 2191)]
HEAD_MASKS = ["none", "ranges", "empty", "full"]
HEAD_SCALE = 100.0
CE_BC = [(1, 1), (3, 5), (4, 64), (7, 65), (65, 200), (256, 1000), (300, 2191)]
CE_KINDS = ["randn", "mag100"]

# The project's own bounds for the same arithmetic (the tests they come from are named in the GPU tests that use them).
HEAD_TOL = 1e-5          # logits / dimg / dtxt against float64, relative to max|ref|
SGEMM_TOL = 2e-5         # fp32 GEMM with fp32 accumulation
LN_TOL = 1e-5            # LayerNorm fp32 rows
REDUCE_TOL = 1e-6        # sums of fp32 rows
ATTN_TOL = {torch.float16: 2e-3 * 3, torch.bfloat16: 1.6e-2 * 3}   # TOL[dtype] * 3 of test_attention_fwd_bwd

# Cross-entropy: the kernel uses the fast exp / log intrinsics and nobody had measured it.  The bound is the error of a plain fp32
# torch implementation of the same formulae (ce_fp32 below) against the float64 reference on the test's own inputs, times 4 (two ~2-ulp
# intrinsics and another summation order).  Measured on the CPU over CE_BC x CE_KINDS x {hard, soft}:
#   loss    (relative to max(1, loss)):  largest fp32 error 1.212e-7, at (65, 200) "mag100" soft labels  -> bound 4.85e-7
#   dlogits (relative to max|ref|):      largest fp32 error 3.950e-6, at (7, 65) "mag100" hard labels    -> bound 1.58e-5
# (the largest shape, (300, 2191): 9.3e-8 / 1.25e-6 at "mag100"; the unit-scale logits stay below 1e-7 / 5e-7 everywhere)
# tests/test_head_ref.py::test_ce_bounds_are_four_times_the_fp32_host_error re-measures both and holds the constants to them.
CE_LOSS_TOL = 4.85e-7
CE_DLOGITS_TOL = 1.58e-5


def rel(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------ head
def head_inputs(e, B, C, mask):
    """img [B, e] (x3), txt [C, e] (x0.02), dlogits [B, C], and the task ranges (lo, hi) int32 [B] or (None, None)."""
    g = torch.Generator().manual_seed(1000 * e + 7 * B + C + HEAD_MASKS.index(mask))
    img = torch.randn(B, e, generator=g) * 3
    txt = torch.randn(C, e, generator=g) * 0.02
    dl = torch.randn(B, C, generator=g)
    if mask == "none":
        return img, txt, dl, None, None
    if mask == "full":
        lo, hi = torch.zeros(B, dtype=torch.int32), torch.full((B,), C, dtype=torch.int32)
    else:
        a = torch.randint(0, C + 1, (B,), generator=g)
        b = torch.randint(0, C + 1, (B,), generator=g)
        lo, hi = torch.minimum(a, b).int(), torch.maximum(a, b).int()
        if mask == "empty":
            lo[B // 2] = hi[B // 2] = C // 2        # one image with no class at all
        else:
            hi = torch.where(hi == lo, torch.clamp(lo + 1, max=C), hi).int()
            lo = torch.where(hi == lo, lo - 1, lo).int()
    return img, txt, dl, lo, hi


def mask01(lo, hi, B, C):
    if lo is None:
        return torch.ones(B, C, dtype=torch.float64)
    c = torch.arange(C).view(1, C)
    return ((c >= lo.view(B, 1)) & (c < hi.view(B, 1))).double()


def head_ref(img, txt, scale, dl, lo=None, hi=None, dtype=torch.float64):
    """Normalise-and-dot logits with the 0/1 mask and their gradients with respect to the UN-normalised features, written out:
    logits = scale * (img / |img|) (txt / |txt|)^T * m;  d imn = scale (dl m) txn;  d img = (d imn - imn (imn . d imn)) / |img|."""
    img, txt, dl = img.to(dtype), txt.to(dtype), dl.to(dtype)
    B, C = dl.shape
    m = mask01(lo, hi, B, C).to(dtype)
    ni, nt = (img * img).sum(-1, keepdim=True).sqrt(), (txt * txt).sum(-1, keepdim=True).sqrt()
    imn, txn = img / ni, txt / nt
    logits = scale * (imn @ txn.t()) * m
    dlm = torch.where(m > 0, dl, torch.zeros_like(dl))      # outside the range dlogits is not read at all
    dimn, dtxn = scale * (dlm @ txn), scale * (dlm.t() @ imn)
    dimg = (dimn - imn * (imn * dimn).sum(-1, keepdim=True)) / ni
    dtxt = (dtxn - txn * (txn * dtxn).sum(-1, keepdim=True)) / nt
    return logits, dimg, dtxt


def argmax_rows_to_compare(logits64, scale, lo=None, hi=None):
    """Rows of a device-computed logits matrix whose arg-max is a fair question: the float64 top-2 gap is at least 2e-5 * scale (the
    logits themselves are held to 1e-5 * max|ref| <= 1e-5 * scale).  The entries outside a task range are exactly 0.0 on both sides, so
    they count as ONE candidate, at their first index: a masked row whose own logits are all clearly negative stays in the comparison."""
    B, C = logits64.shape
    m = mask01(lo, hi, B, C) > 0
    cand = torch.where(m, logits64, torch.full_like(logits64, -math.inf))
    cand = torch.cat([cand, torch.where(m.all(-1, keepdim=True), -math.inf, 0.0).double()], dim=-1)     # the one zero, if any
    if cand.shape[1] < 2:
        return torch.ones(B, dtype=torch.bool)
    top = cand.topk(2, dim=-1).values
    return (top[:, 0] - top[:, 1]) >= 2e-5 * scale


# ------------------------------------------------------------------------------------------------ cross-entropy
def ce_inputs(B, C, kind, soft):
    """fp32 logits [B, C] and labels (int64 [B], or fp32 [B, C]); rows with exact ties are planted where C leaves room for them."""
    g = torch.Generator().manual_seed(17 * B + C + (5 if soft else 0) + (11 if kind == "mag100" else 0))
    if kind == "mag100":
        z = (torch.rand(B, C, generator=g) * 2 - 1) * 100.0          # cosines times the largest logit scale
    else:
        z = torch.randn(B, C, generator=g) * 2
    hard = torch.randint(0, C, (B,), generator=g)
    r = 0
    if C >= 3 and B > r:          # a masked row: zeros outside the task range [1, C - 1), in-task logits all negative -> arg-max 0
        z[r] = 0.0
        z[r, 1:C - 1] = -z.new_empty(C - 2).uniform_(0.5, 9.0, generator=g)
        hard[r] = 0
        r += 1
    if C >= 2 and B > r:          # two equal maxima 1 apart
        c0 = (C - 2) // 2
        z[r, c0] = z[r, c0 + 1] = float(z[r].max()) + 1.5
        hard[r] = c0
        r += 1
    if C >= 66 and B > r:         # two equal maxima 64 apart: the same lane of the wave holds both
        c0 = (C - 65) // 3
        z[r, c0] = z[r, c0 + 64] = float(z[r].max()) + 0.75
        hard[r] = c0
        r += 1
    if C >= 66 and B > r:         # ... and the label on the SECOND of them: a miss under the first-maximum rule
        c0 = 1
        z[r, c0] = z[r, c0 + 64] = float(z[r].max()) + 0.25
        hard[r] = c0 + 64
        r += 1
    if not soft:
        return z, hard
    y = torch.zeros(B, C)
    for b in range(B):
        k = b % 5
        if k == 0:
            y[b, hard[b]] = 1.0                                    # one-hot
        elif k == 4:
            pass                                                   # a row of zeros
        else:
            p = torch.rand(C, generator=g)
            p[hard[b]] += 0.5
            y[b] = p / p.sum() * (1.0, 0.5, 3.0)[k - 1]            # normalised, summing to 0.5, summing to 3
    return z, y


def ce_ref(z, label, dtype=torch.float64):
    """(loss, dlogits, ncorrect): mean over the rows of sum_c y (lse - z), dlogits = (softmax * sum(y) - y) / B, and the count of rows
    whose arg-max (numpy.argmax: the first maximum wins) is the label (arg-max of a soft label row)."""
    B, C = z.shape
    zz = z.to(dtype)
    if label.dtype == torch.int64:
        y = torch.zeros(B, C, dtype=dtype)
        y[torch.arange(B), label] = 1.0
        target = label.numpy()
    else:
        y = label.to(dtype)
        target = np.argmax(label.numpy(), axis=-1)
    m = zz.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(zz - m).sum(-1, keepdim=True))
    loss = (y * (lse - zz)).sum(-1).sum() / B
    dl = (torch.exp(zz - lse) * y.sum(-1, keepdim=True) - y) / B
    ncorrect = int((np.argmax(z.numpy(), axis=-1) == target).sum())
    return loss, dl, ncorrect


def ce_fp32(z, label):
    """The same formulae in plain fp32 torch: the yardstick of the cross-entropy bound."""
    return ce_ref(z, label, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ attention, CLS query only
def attn_cls_inputs(N, L, H, dtype, seed=0):
    """qkv [N*L, 3*H*64] and do_cls [N, H*64] rounded to the 16-bit type, and lse [N*H*L] fp32 / o_cls [N, H*64] (16-bit) from the
    float64 forward of those rounded inputs for query 0 of every sequence.  The lse of the other queries is never read: NaN there."""
    g = torch.Generator().manual_seed(97 * L + 13 * N + H + seed)
    d = H * 64
    qkv = torch.randn(N * L, 3 * d, generator=g).to(dtype)
    do = torch.randn(N, d, generator=g).to(dtype)
    x = qkv.double().reshape(N, L, 3, H, 64)
    s0 = torch.einsum("nhe,nlhe->nhl", x[:, 0, 0], x[:, :, 1]) / 8.0         # [N, H, L]: query 0 against every key
    lse0 = torch.logsumexp(s0, dim=-1)                                       # [N, H]
    o0 = torch.einsum("nhl,nlhe->nhe", torch.softmax(s0, dim=-1), x[:, :, 2])
    lse = torch.full((N, H, L), float("nan"))
    lse[:, :, 0] = lse0.float()
    return qkv, do, lse.reshape(-1), o0.reshape(N, d).to(dtype)


def attn_bwd_cls_ref(qkv, o_cls, do_cls, lse, N, L, H):
    """dqkv [N*L, 3*H*64] in float64 from the formulae of the kernel's header comment, per (sequence, head):
    delta = dO.O,  p_j = exp(q.k_j / 8 - lse),  dp_j = dO.v_j,  ds_j = p_j (dp_j - delta) / 8,
    dV_j = p_j dO,  dK_j = ds_j q,  dQ_0 = sum_j ds_j k_j,  dQ_{i>0} = 0."""
    d = H * 64
    x = qkv.double().reshape(N, L, 3, H, 64)
    q0, k, v = x[:, 0, 0], x[:, :, 1], x[:, :, 2]                   # [N, H, 64], [N, L, H, 64] x 2
    do, o = do_cls.double().reshape(N, H, 64), o_cls.double().reshape(N, H, 64)
    l0 = lse.double().reshape(N, H, L)[:, :, 0]                     # [N, H]
    delta = (do * o).sum(-1)                                        # [N, H]
    p = torch.exp(torch.einsum("nhe,nlhe->nlh", q0, k) / 8.0 - l0.unsqueeze(1))
    dp = torch.einsum("nhe,nlhe->nlh", do, v)
    ds = p * (dp - delta.unsqueeze(1)) / 8.0                        # [N, L, H]
    out = torch.zeros(N, L, 3, H, 64, dtype=torch.float64)
    out[:, :, 2] = p.unsqueeze(-1) * do.unsqueeze(1)
    out[:, :, 1] = ds.unsqueeze(-1) * q0.unsqueeze(1)
    out[:, 0, 0] = torch.einsum("nlh,nlhe->nhe", ds, k)
    return out.reshape(N * L, 3 * d)


# ------------------------------------------------------------------------------------------------ gradient scale
def scale_rule(v, target):
    """(scale, 1 / scale) as Python floats: scale = 2^k, k = exponent(target) - exponent(amax|v|) from math.frexp, clamped to [-60, 60];
    1 when amax is 0, inf or NaN."""
    amax = float(np.max(np.abs(np.asarray(v, dtype=np.float32)))) if len(v) else 0.0     # numpy's max propagates NaN
    if not (amax > 0.0 and math.isfinite(amax)):
        return 1.0, 1.0
    k = math.frexp(float(target))[1] - math.frexp(amax)[1]
    k = max(-60, min(60, k))
    return math.ldexp(1.0, k), math.ldexp(1.0, -k)


# ------------------------------------------------------------------------------------------------ data movement / LayerNorm rows
def layernorm_rows(x, gamma, beta, eps=1e-5):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def assemble_tokens_ref(pe, cls, pos, gamma, beta, batch, vpt=None, vmask=None):
    """(x float64 [batch, 1 + n_vpt + G2, d], is_prompt bool [1 + n_vpt + G2]); the prompt rows are exact fp32 products."""
    d = pe.shape[1]
    G2 = pe.shape[0] // batch
    n = 0 if vpt is None else vpt.shape[0]
    x = torch.zeros(batch, 1 + n + G2, d, dtype=torch.float64)
    x[:, 0] = layernorm_rows((cls + pos[0]).double().expand(batch, d), gamma, beta)      # fp32 sums first: cls + pos is ONE fp32 add
    x[:, 1 + n:] = layernorm_rows(pe.view(batch, G2, d) + pos[1:], gamma, beta)
    if n:
        rows = vpt.unsqueeze(0).expand(batch, n, d)
        x[:, 1:1 + n] = (rows * vmask if vmask is not None else rows).double()             # fp32 product, as the kernel forms it
    is_prompt = torch.zeros(1 + n + G2, dtype=torch.bool)
    is_prompt[1:1 + n] = True
    return x, is_prompt
