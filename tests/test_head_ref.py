"""CPU checks of tests/head_ref.py: every float64 reference the GPU tests of the dense head, the loss and the fp32 glue compare a
kernel with is pinned here to torch autograd in float64 or to oracle/clip_oracle.py, and the bounds those tests do not inherit from
the project are derived from the error of a plain fp32 host implementation.  No GPU."""
import math

import numpy as np
import pytest
import torch

from oracle import clip_oracle as O
from tests import head_ref as R


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("mask", R.HEAD_MASKS)
@pytest.mark.parametrize("e,B,C", [(64, 1, 1), (128, 5, 7), (576, 17, 255), (1024, 13, 300)])
def test_head_ref_is_autograd_and_oracle(e, B, C, mask):
    img, txt, dl, lo, hi = R.head_inputs(e, B, C, mask)
    logits, dimg, dtxt = R.head_ref(img, txt, R.HEAD_SCALE, dl, lo, hi)
    m = R.mask01(lo, hi, B, C)
    if mask == "empty":
        assert float(m[B // 2].sum()) == 0.0
    if mask == "full":
        assert bool((m == 1).all())
    # autograd in float64
    i64, t64 = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    want = R.HEAD_SCALE * (i64 / i64.norm(dim=-1, keepdim=True)) @ (t64 / t64.norm(dim=-1, keepdim=True)).t() * m
    want.backward(dl.double())
    assert R.rel(logits, want.detach()) <= 1e-14
    assert float((dimg - i64.grad).abs().max()) <= 1e-13 * max(float(i64.grad.abs().max()), 1e-300)
    assert float((dtxt - t64.grad).abs().max()) <= 1e-13 * max(float(t64.grad.abs().max()), 1e-300)
    # the project's oracle, in float64
    ol, ctx = O.logits_fwd(img.double(), txt.double(), R.HEAD_SCALE, None if lo is None else m)
    oi, ot = O.logits_bwd(dl.double(), ctx)
    assert R.rel(logits, ol) <= 1e-14 and torch.equal(logits == 0, ol == 0)
    assert float((dimg - oi).abs().max()) <= 1e-13 * max(float(oi.abs().max()), 1e-300)
    assert float((dtxt - ot).abs().max()) <= 1e-13 * max(float(ot.abs().max()), 1e-300)
    # outside the ranges dlogits is not read: NaN there changes nothing
    if lo is not None:
        dl_nan = torch.where(m > 0, dl, torch.full_like(dl, float("nan")))
        _, di2, dt2 = R.head_ref(img, txt, R.HEAD_SCALE, dl_nan, lo, hi)
        assert torch.equal(di2, dimg) and torch.equal(dt2, dtxt)


def test_head_fp32_host_error_stays_inside_the_project_bound():
    """The issue's question before the GPU run: does a plain fp32 host implementation of the same sums already exceed
    1e-5 * max|ref| at the longest reductions (2191 rows of e = 1024)?  It does not, at any listed shape, so every shape keeps
    HEAD_TOL (largest fp32 host error seen here: below 2e-6)."""
    worst = 0.0
    for e in (64, 1024):
        for B, C in R.HEAD_BC:
            for mask in ("none", "ranges"):
                img, txt, dl, lo, hi = R.head_inputs(e, B, C, mask)
                ref = R.head_ref(img, txt, R.HEAD_SCALE, dl, lo, hi)
                f32 = R.head_ref(img, txt, R.HEAD_SCALE, dl, lo, hi, dtype=torch.float32)
                for a, b in zip(f32, ref):
                    if float(b.abs().max()) > 0:
                        worst = max(worst, R.rel(a, b))
    assert worst * 4 <= R.HEAD_TOL, worst


def test_head_argmax_exclusion_stays_below_one_percent():
    """Rows left out of the head tests' arg-max comparison (float64 top-2 gap below 2e-5 * scale): at most 1 % of all rows over the
    seeds the GPU test uses."""
    rows = out = 0
    for e in R.HEAD_EMBED:
        for B, C in R.HEAD_BC:
            for mask in R.HEAD_MASKS:
                img, txt, dl, lo, hi = R.head_inputs(e, B, C, mask)
                logits, _, _ = R.head_ref(img, txt, R.HEAD_SCALE, dl, lo, hi)
                keep = R.argmax_rows_to_compare(logits, R.HEAD_SCALE, lo, hi)
                rows += B
                out += int((~keep).sum())
    assert out <= 0.01 * rows, (out, rows)


# ------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 5), (7, 65), (65, 200)])
def test_ce_ref_is_autograd_and_oracle(B, C, soft):
    z, label = R.ce_inputs(B, C, "randn", soft)
    loss, dl, nc = R.ce_ref(z, label)
    z64 = z.double().requires_grad_(True)
    logp = torch.log_softmax(z64, dim=-1)
    if soft:
        want = -(label.double() * logp).sum(-1).mean()          # rows that do not sum to 1 included: the kernel's formula
    else:
        want = torch.nn.functional.cross_entropy(z64, label)
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-13 * max(1.0, abs(float(want)))
    assert float((dl - z64.grad).abs().max()) <= 1e-14
    ol, od = O.cross_entropy_fwd_bwd(z.double(), label if not soft else label.double())
    assert abs(float(loss) - float(ol)) <= 1e-12 * max(1.0, abs(float(ol)))
    assert float((dl - od.double()).abs().max()) <= 1e-7      # the oracle casts soft labels to fp32 and works there
    # first maximum wins
    target = label.numpy() if not soft else np.argmax(label.numpy(), -1)
    assert nc == sum(int(np.argmax(z[b].numpy()) == target[b]) for b in range(B))


def test_ce_inputs_hold_the_planted_ties():
    z, label = R.ce_inputs(65, 200, "randn", False)
    assert int(np.argmax(z[0].numpy())) == 0 and float(z[0].max()) == 0.0 and bool((z[0, 1:199] < 0).all())
    for r, gap in ((1, 1), (2, 64), (3, 64)):
        top = torch.nonzero(z[r] == z[r].max()).flatten().tolist()
        assert len(top) == 2 and top[1] - top[0] == gap
    assert int(label[3]) == int(np.argmax(z[3].numpy())) + 64          # a miss under the first-maximum rule
    _, y = R.ce_inputs(65, 200, "mag100", True)
    sums = y.sum(-1)
    assert float(sums[4]) == 0.0 and abs(float(sums[2]) - 0.5) < 1e-6 and abs(float(sums[3]) - 3.0) < 1e-5
    assert float(y[0].max()) == 1.0 and float(sums[0]) == 1.0
    assert float(R.ce_inputs(300, 2191, "mag100", False)[0].abs().max()) >= 99.0


def _ce_fp32_errors():
    worst_loss, worst_dl = (0.0, None), (0.0, None)
    for B, C in R.CE_BC:
        for kind in R.CE_KINDS:
            for soft in (False, True):
                z, label = R.ce_inputs(B, C, kind, soft)
                loss, dl, _ = R.ce_ref(z, label)
                l32, d32, _ = R.ce_fp32(z, label)
                el = abs(float(l32) - float(loss)) / max(1.0, abs(float(loss)))
                ed = R.rel(d32, dl) if float(dl.abs().max()) > 0 else 0.0
                if el > worst_loss[0]:
                    worst_loss = (el, (B, C, kind, soft))
                if ed > worst_dl[0]:
                    worst_dl = (ed, (B, C, kind, soft))
    return worst_loss, worst_dl


def test_ce_bounds_are_four_times_the_fp32_host_error():
    """CE_LOSS_TOL / CE_DLOGITS_TOL are 4 x the error of plain fp32 torch against float64 on the GPU test's own inputs (head_ref.py
    records the figures).  An fp32 sum may be ordered differently on another host, so the constants are held to the re-measured
    error within a factor of 1.5 either way, not to the digit."""
    (el, where_l), (ed, where_d) = _ce_fp32_errors()
    print(f"fp32 host error: loss {el:.3e} at {where_l}, dlogits {ed:.3e} at {where_d}")
    assert 4 * el / 1.5 <= R.CE_LOSS_TOL <= 4 * el * 1.5, (el, where_l)
    assert 4 * ed / 1.5 <= R.CE_DLOGITS_TOL <= 4 * ed * 1.5, (ed, where_d)


# ------------------------------------------------------------------------------------------------ attention, CLS query only
@pytest.mark.parametrize("N,L,H", [(1, 1, 1), (3, 5, 2), (2, 65, 3)])
def test_attn_bwd_cls_ref_is_autograd_and_oracle(N, L, H):
    d = H * 64
    qkv, do, lse, o_cls = R.attn_cls_inputs(N, L, H, torch.float16)
    # float64 lse / O here: the reference is exact in its inputs, the GPU test feeds it the rounded ones the kernel reads
    x = qkv.double().reshape(N, L, 3 * d).requires_grad_(True)
    q, k, v = (t.reshape(N, L, H, 64).permute(0, 2, 1, 3) for t in x.split(d, dim=-1))
    s = q @ k.transpose(-1, -2) / 8.0
    o = torch.softmax(s, -1) @ v                                             # [N, H, L, 64]
    lse64 = torch.logsumexp(s, -1).reshape(-1).detach()
    o0 = o[:, :, 0].reshape(N, d)
    got = R.attn_bwd_cls_ref(qkv, o0.detach(), do, lse64, N, L, H)
    (o0 * do.double()).sum().backward()
    assert R.rel(got, x.grad.reshape(N * L, 3 * d)) <= 1e-13
    assert bool((got.reshape(N, L, 3 * d)[:, 1:, :d] == 0).all())
    # the project's oracle: full attention backward with a gradient on query 0 only
    dof = torch.zeros(N, H, L, 64, dtype=torch.float64)
    dof[:, :, 0] = do.double().reshape(N, H, 64)
    _, p = O.attention_fwd(q.detach(), k.detach(), v.detach(), False)
    dq, dk, dv = O.attention_bwd(dof, q.detach(), k.detach(), v.detach(), p)
    want = torch.cat([t.permute(0, 2, 1, 3).reshape(N * L, d) for t in (dq, dk, dv)], dim=-1)
    assert R.rel(got, want) <= 1e-13
    # what attn_cls_inputs hands the kernel is this forward, rounded
    lse0, want0 = lse.reshape(N, H, L)[:, :, 0].double(), lse64.reshape(N, H, L)[:, :, 0]
    assert float((lse0 - want0).abs().max()) <= 1e-6 * max(1.0, float(want0.abs().max()))
    assert L == 1 or bool(torch.isnan(lse.reshape(N, H, L)[:, :, 1:]).all())
    assert R.rel(o_cls, o0.detach()) <= 2e-3


# ------------------------------------------------------------------------------------------------ gradient scale
def test_scale_rule():
    f = np.float32
    assert R.scale_rule([f(1.0)], 64.0) == (64.0, 1 / 64.0)                 # frexp(1) = (0.5, 1), frexp(64) = (0.5, 7)
    assert R.scale_rule([f(0.75), f(-1.5)], 64.0) == (64.0, 1 / 64.0)               # frexp(1.5) = (0.75, 1)
    assert R.scale_rule([f(0.75), f(-2.0)], 64.0) == (32.0, 1 / 32.0)
    assert R.scale_rule([f(63.9)], 128.0) == (4.0, 0.25)
    assert R.scale_rule([f(0), f(-0.0)], 64.0) == (1.0, 1.0)
    assert R.scale_rule([f(1), f("inf")], 64.0) == (1.0, 1.0)
    assert R.scale_rule([f(1), f("nan"), f(2)], 64.0) == (1.0, 1.0)
    assert R.scale_rule([f(1e-40)], 64.0) == (2.0 ** 60, 2.0 ** -60)        # a denormal amax: clamped
    assert R.scale_rule([f(3e38)], 64.0) == (2.0 ** -60, 2.0 ** 60)
    for amax in (3e-5, 0.02, 1.0, 777.0):
        s, inv = R.scale_rule([f(amax)], 64.0)
        assert 64.0 <= float(f(amax)) * s < 128.0 and s * inv == 1.0 and math.frexp(s)[0] == 0.5


# ------------------------------------------------------------------------------------------------ row reductions
def test_row_sum_fp32_host_error_stays_inside_the_project_bound():
    """reduce_prompt_rows / gather_ctx_grad add up to 256 fp32 rows; REDUCE_TOL = 1e-6 * max|ref| comes from a 37-row test.  A plain
    fp32 host sum over 256 rows does not exceed it (torch.sum: 1.5e-7; one add after the other, the least careful order: 5.7e-7; the
    kernel's 16 partials is 1.9e-7), with and without the dropout-mask product, so the longest sums keep the project's bound."""
    g = torch.Generator().manual_seed(256)
    rows = torch.randn(256, 16, 1024, generator=g)
    vmask = (torch.rand(256, 16, 1024, generator=g) > 0.1).float() / 0.9
    for x in (rows, rows * vmask):
        want = x.double().sum(0)
        seq = torch.zeros(16, 1024)
        for b in range(256):
            seq = seq + x[b]
        assert max(R.rel(x.sum(0), want), R.rel(seq, want)) <= R.REDUCE_TOL


# ------------------------------------------------------------------------------------------------ token assembly
def test_assemble_tokens_ref_is_layer_norm_and_rows():
    g = torch.Generator().manual_seed(3)
    B, G2, d, n = 3, 4, 192, 2
    pe, cls, pos = torch.randn(B * G2, d, generator=g), torch.randn(d, generator=g), torch.randn(1 + G2, d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    vpt, vmask = torch.randn(n, d, generator=g), (torch.rand(B, n, d, generator=g) > 0.3).float() / 0.7
    x, is_prompt = R.assemble_tokens_ref(pe, cls, pos, gamma, beta, B, vpt, vmask)
    assert is_prompt.tolist() == [False, True, True, False, False, False, False]
    seq = torch.cat([(cls + pos[0]).expand(B, 1, d), pe.view(B, G2, d) + pos[1:]], dim=1).double()
    want = torch.nn.functional.layer_norm(seq, (d,), gamma.double(), beta.double(), 1e-5)
    assert R.rel(x[:, ~is_prompt], want) <= 1e-13
    assert torch.equal(x[:, is_prompt].float(), vpt.unsqueeze(0) * vmask)
    y, _ = O.layernorm_fwd(seq.float(), gamma, beta)
    assert R.rel(x[:, ~is_prompt], y) <= 1e-5
