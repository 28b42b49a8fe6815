"""Kernel-level float64 parity of the dense head and the loss (-m gpu): normalize_rows + logits with the lo/hi task mask,
logits_bwd<IMG> / <!IMG>, ce_rows + ce_mean, and sgemm_bt (the two fp32 projections next to the logits and their backward).  The
references and the seeded inputs are tests/head_ref.py (pinned to autograd / the oracle on the CPU by tests/test_head_ref.py); every
kernel runs twice and the two results must be bit-identical."""
import numpy as np
import pytest
import torch

from tests import head_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _engine(e, cache={}):
    """The head needs no weights: an Engine on an arch with the wanted embed_dim is enough."""
    if e not in cache:
        from mvlpt_amd.engine import Engine
        from mvlpt_amd.weights import ClipArch
        arch = ClipArch(name=f"head-e{e}", embed_dim=e, image_resolution=32, vision_layers=1, vision_width=128, vision_patch_size=16,
                        context_length=77, vocab_size=64, transformer_width=128, transformer_heads=2, transformer_layers=1)
        cache[e] = Engine(arch, device=DEV)
    return cache[e]


def _dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("B,C", R.HEAD_BC)
@pytest.mark.parametrize("e", R.HEAD_EMBED)
def test_head_fwd_bwd_against_float64(e, B, C):
    """HEAD_TOL = 1e-5 * max|ref| is the bound of test_grouped_head_fwd_bwd_against_float64 / test_ranged_head_fwd_bwd_against_float64;
    a plain fp32 host implementation stays 4x inside it at every shape here (tests/test_head_ref.py), so no shape gets another."""
    eng = _engine(e)
    for mask in R.HEAD_MASKS:
        img, txt, dl, lo, hi = R.head_inputs(e, B, C, mask)
        want, dimg64, dtxt64 = R.head_ref(img, txt, R.HEAD_SCALE, dl, lo, hi)
        m = R.mask01(lo, hi, B, C) > 0
        runs = []
        for _ in range(2):
            logits = eng.logits_fwd(_dev(img), _dev(txt), R.HEAD_SCALE, _dev(lo), _dev(hi))
            dimg, dtxt = eng.logits_bwd(_dev(dl))
            runs.append((logits.cpu(), dimg.cpu(), dtxt.cpu()))
        for a, b in zip(*runs):
            assert torch.equal(a, b), f"{mask}: not bit-stable from run to run"
        logits, dimg, dtxt = runs[0]
        # either gradient alone is the same kernel on the same data
        only_img, none_t = eng.logits_bwd(_dev(dl), need_img=True, need_txt=False)
        none_i, only_txt = eng.logits_bwd(_dev(dl), need_img=False, need_txt=True)
        assert none_t is None and none_i is None
        assert torch.equal(only_img.cpu(), dimg) and torch.equal(only_txt.cpu(), dtxt)
        # outside the range: logits exactly 0.0, and dlogits never read (NaN there changes nothing)
        assert bool((logits[~m] == 0).all())
        if lo is not None:
            dl_nan = torch.where(m, dl, torch.full_like(dl, float("nan")))
            di2, dt2 = eng.logits_bwd(_dev(dl_nan))
            assert torch.equal(di2.cpu(), dimg) and torch.equal(dt2.cpu(), dtxt), f"{mask}: dlogits outside the range was read"
        assert bool(torch.isfinite(logits).all() and torch.isfinite(dimg).all() and torch.isfinite(dtxt).all())
        errs = {}
        for name, got, ref in (("logits", logits, want), ("dimg", dimg, dimg64), ("dtxt", dtxt, dtxt64)):
            scale = float(ref.abs().max())
            errs[name] = float((got.double() - ref).abs().max()) / scale if scale > 0 else float(got.abs().max())
        print(f"head e={e} B={B} C={C} {mask}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for name, v in errs.items():
            assert v <= R.HEAD_TOL, f"{mask}: {name} {v:.3e}"
        # the arg-max question on device-computed logits (rows with a float64 top-2 gap below 2e-5 * scale left out)
        keep = R.argmax_rows_to_compare(want, R.HEAD_SCALE, lo, hi)
        got_arg, want_arg = np.argmax(logits.numpy(), -1), np.argmax(want.numpy(), -1)
        assert np.array_equal(got_arg[keep.numpy()], want_arg[keep.numpy()]), f"{mask}: arg-max differs"


def test_head_backward_refuses_an_embed_dim_it_cannot_hold():
    """logits_bwd keeps a feature row in 2 x 64 lanes x 8 columns: e = 1088 must fail loudly, not return garbage."""
    eng = _engine(1088)
    g = torch.Generator().manual_seed(1088)
    img, txt, dl = torch.randn(3, 1088, generator=g), torch.randn(5, 1088, generator=g), torch.randn(3, 5, generator=g)
    logits = eng.logits_fwd(_dev(img), _dev(txt), R.HEAD_SCALE)
    want, _, _ = R.head_ref(img, txt, R.HEAD_SCALE, dl)
    assert R.rel(logits, want) <= R.HEAD_TOL                       # the forward has no such limit
    with pytest.raises(RuntimeError):
        eng.logits_bwd(_dev(dl))


# ------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("kind", R.CE_KINDS)
@pytest.mark.parametrize("B,C", R.CE_BC)
def test_cross_entropy_against_float64(B, C, kind, soft):
    """The same fp32 logits go to the kernel and to the reference, so arg-max (first maximum wins) is an exact question and ncorrect
    must equal the reference count.  Bounds: CE_LOSS_TOL / CE_DLOGITS_TOL of tests/head_ref.py, 4 x the fp32 host error."""
    eng = _engine(64)
    z, label = R.ce_inputs(B, C, kind, soft)
    loss64, dl64, nc = R.ce_ref(z, label)
    runs = []
    for _ in range(2):
        loss, dl, ncorrect = eng.cross_entropy(_dev(z), _dev(label))
        runs.append((loss.cpu(), dl.cpu(), ncorrect.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "cross-entropy is not bit-stable from run to run"
    loss, dl, ncorrect = runs[0]
    loss_ng, dl_ng, nc_ng = eng.cross_entropy(_dev(z), _dev(label), need_grad=False)
    assert dl_ng is None and torch.equal(loss_ng.cpu(), loss) and torch.equal(nc_ng.cpu(), ncorrect)
    e_loss = abs(float(loss) - float(loss64)) / max(1.0, abs(float(loss64)))
    scale = float(dl64.abs().max())
    e_dl = float((dl.double() - dl64).abs().max()) / scale if scale > 0 else float(dl.abs().max())
    print(f"ce B={B} C={C} {kind} {'soft' if soft else 'hard'}: loss {float(loss):.6f} (ref {float(loss64):.6f}) err {e_loss:.2e}, "
          f"dlogits err {e_dl:.2e}, ncorrect {float(ncorrect):.0f} (ref {nc})")
    assert float(ncorrect) == nc
    assert e_loss <= R.CE_LOSS_TOL
    assert e_dl <= R.CE_DLOGITS_TOL


# ------------------------------------------------------------------------------------------------ fp32 GEMM
SGEMM_SHAPES = [(1, 4, 16), (15, 12, 48), (17, 20, 128), (100, 512, 768), (256, 768, 1024), (1000, 1024, 512), (33, 128, 128)]


@pytest.mark.parametrize("M,N,K", SGEMM_SHAPES)
def test_sgemm_bt_against_float64(M, N, K):
    """SGEMM_TOL = 2e-5 * max|ref| is the EPI_STORE32 bound of test_gemm_epilogues.  A and Bt are random and non-symmetric, M != N: a
    transposed or mis-mapped result cannot pass."""
    from mvlpt_amd.engine import op_sgemm_bt
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A, Bt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    want = A.double() @ Bt.double().t()
    alpha = torch.tensor([2.0 ** -7], device=DEV)
    for al, ref in ((None, want), (alpha, want * 2.0 ** -7)):
        a = op_sgemm_bt(_dev(A), _dev(Bt), al).cpu()
        b = op_sgemm_bt(_dev(A), _dev(Bt), al).cpu()
        assert torch.equal(a, b)
        err = R.rel(a, ref)
        print(f"sgemm_bt {M}x{N}x{K} alpha {'2^-7' if al is not None else 'null'}: {err:.2e}")
        assert err <= R.SGEMM_TOL
    # alpha = 2^-7 is exact: the scaled result is the unscaled one, bit for bit
    assert torch.equal(op_sgemm_bt(_dev(A), _dev(Bt), alpha).cpu() * 128.0, op_sgemm_bt(_dev(A), _dev(Bt)).cpu())


@pytest.mark.parametrize("M,N,K", [(16, 16, 24), (16, 16, 8), (16, 6, 16), (16, 17, 32)])
def test_sgemm_bt_refuses_what_it_cannot_compute(M, N, K):
    from mvlpt_amd.engine import op_sgemm_bt
    with pytest.raises(RuntimeError):
        op_sgemm_bt(torch.zeros(M, K, device=DEV), torch.zeros(N, K, device=DEV))
