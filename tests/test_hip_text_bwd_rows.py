"""Gradient length of the text tower (-m gpu): mvlpt_set_text_grad_len / TRAINER.MVLPT.TEXT_GRAD_TO_EOT.

The text backward processes only the leading Lg positions of every sequence: behind a sequence's EOT the gradient is exactly zero
(the only gradient enters at the EOT row, the attention is causal, everything else acts row by row).  The gradient buffers are
compact [C, Lg, .]; the saved forward tensors keep the pitch L and are read through the row map r -> (r // Lg) * L + r % Lg.

1. kernel level: every launch that reads a saved tensor through the map, against a float64 restatement in this file, at the bounds
   the existing kernel tests of the same op use (tests/test_hip_ops.py, tests/test_hip_glue.py);
2. tower level: dctx / dctx_deep with Lg = max(eot) + 1 have the BITS of Lg = L, in every arrangement of the tower;
3. arguments and state."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 2e-3, BF16: 1.6e-2}                 # tests/test_hip_ops.py: output rounding of the 16-bit type
SPLIT_TOL = {F16: 3e-6, BF16: 6e-5}             # ... pair = 22 / 16 significant bits
REDUCE_TOL = 1e-6                               # tests/head_ref.py: sums of fp32 rows
CS, L, LGS = 5, 20, (7, 16, 17, 20)             # C * Lg = 35, 80, 85, 100: no multiple of 128; 7 and 17: no multiple of 16


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _lib():
    from mvlpt_amd import _lib
    return _lib


def _E():
    from mvlpt_amd import engine
    return engine


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _saved_rows(C_, Lg, Ls):
    """Saved-tensor row of every gradient row: the map under test, restated."""
    r = torch.arange(C_ * Lg)
    return (r // Lg) * Ls + r % Lg


# ------------------------------------------------------------------------------------------------ 1a: GELU-backward epilogue
def _quick_gelu_grad64(u):
    s = torch.sigmoid(1.702 * u)
    return s * (1 + 1.702 * u * (1 - s))


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("C_", [CS, 37])          # 37 * 7 = 259, 37 * 17 = 629: more than one row tile, ragged last tile
@pytest.mark.parametrize("Lg", LGS)
def test_gelu_backward_epilogue_reads_u_through_the_row_map(Lg, C_, dtype):
    lib, E = _lib(), _E()
    N, K, M = 256, 128, C_ * Lg
    g = torch.Generator().manual_seed(1000 * Lg + C_)
    A = torch.randn(M, K, generator=g)
    Bt = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    u = torch.randn(C_ * L, N, generator=g).to(dtype)             # saved at the pitch L
    rows = _saved_rows(C_, Lg, L)
    slope = _quick_gelu_grad64(u.double()[rows])
    dt = E._TORCH2DT[dtype]
    # single operands: out16 = acc * QuickGELU'(u)
    A16 = A.to(dtype)
    ref = (A16.double() @ Bt.double().t()) * slope
    out = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
    A_d, Bt_d, u_d = A16.to(DEV), Bt.to(DEV), u.to(DEV)
    lib.check(lib.lib.mvlpt_op_gemm_gelubwd_rows(dt, lib.EPI_GELUBWD, _ptr(A_d), _ptr(Bt_d), M, N, K, _ptr(u_d), _ptr(out), 0, 0, 0, 0, 0, 0,
                                                 Lg, L, None), None, "gemm_gelubwd_rows")
    e1 = _rel(out, ref)
    # pair operands: out [M, 2N] = split(acc * QuickGELU'(u))
    A2 = E.split_pair(A, dtype).to(DEV)
    ref2 = (E.join_pair(A2.cpu()).double() @ Bt.double().t()) * slope
    out2 = torch.full((M, 2 * N), float("nan"), dtype=dtype, device=DEV)
    lib.check(lib.lib.mvlpt_op_gemm_gelubwd_rows(dt, lib.EPI_GELUBWD_SPLIT, _ptr(A2), _ptr(Bt_d), M, N, K, _ptr(u_d), _ptr(out2), 1, 0, 0, 0, 0, 0,
                                                 Lg, L, None), None, "gemm_gelubwd_rows split")
    torch.cuda.synchronize()
    e2 = _rel(E.join_pair(out2.cpu()), ref2)
    print(f"gelubwd rows C={C_} Lg={Lg} {dtype}: single {e1:.2e}, pair {e2:.2e}")
    assert e1 < TOL[dtype], e1
    assert e2 < 2e-6 * (1 if dtype == F16 else 40), e2        # (test_gemm_split_epilogues: fp32-level, the device's exp / rcp)


def test_gelu_backward_row_map_is_checked():
    lib, E = _lib(), _E()
    t = torch.zeros(64, 256, dtype=F16, device=DEV)
    for M, Lg, Ls in ((60, 2, 20), (60, 7, 20), (60, 20, 10)):        # sequences shorter than 3, M no whole sequences, pitch < length
        rc = lib.lib.mvlpt_op_gemm_gelubwd_rows(E._TORCH2DT[F16], lib.EPI_GELUBWD, _ptr(t), _ptr(t), M, 256, 128, _ptr(t), _ptr(t),
                                                0, 0, 0, 0, 0, 0, Lg, Ls, None)
        assert rc != 0, (M, Lg, Ls)


# ------------------------------------------------------------------------------------------------ 1b: LayerNorm backward
def _ln_bwd64(dy, x, gamma, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat, gg = (x - mean) * rstd, dy * gamma
    return rstd * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))


@pytest.mark.parametrize("C_,d", [(CS, 128), (CS, 512), (300, 256)])        # 300 * 20 = 6000 saved rows: the grid-stride kernel
@pytest.mark.parametrize("Lg", LGS)
def test_layernorm_backward_reads_x_through_the_row_map(Lg, C_, d):
    lib, E = _lib(), _E()
    rows = C_ * Lg
    g = torch.Generator().manual_seed(100 * Lg + d)
    x = torch.randn(C_ * L, d, generator=g) * 3 + 0.5             # saved at the pitch L
    gamma = 1 + 0.1 * torch.randn(d, generator=g)
    dy, resid = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    ref = resid.double() + _ln_bwd64(dy.double(), x.double()[_saved_rows(C_, Lg, L)], gamma.double())
    x_d, g_d, dy_d, r_d = (t.to(DEV) for t in (x, gamma, dy, resid))
    for dtype in (F16, BF16):
        out32 = torch.full((rows, d), float("nan"), device=DEV)
        pair = torch.full((rows, 2 * d), float("nan"), dtype=dtype, device=DEV)
        lib.check(lib.lib.mvlpt_op_layernorm_bwd_rows(E._TORCH2DT[dtype], _ptr(dy_d), lib.DT_F32, _ptr(x_d), _ptr(g_d), _ptr(r_d), _ptr(out32),
                                                      _ptr(pair), rows, d, 1, Lg, L, None), None, "layernorm_bwd_rows")
        torch.cuda.synchronize()
        e32, e16 = _rel(out32, ref), _rel(E.join_pair(pair.cpu()), out32)
        print(f"ln_bwd rows C={C_} d={d} Lg={Lg} {dtype}: fp32 {e32:.2e}, pair against it {e16:.2e}")
        assert e32 < 2e-5 and e16 < SPLIT_TOL[dtype], (e32, e16)         # test_layernorm_split_outputs
    # in place on the residual, as the towers run it
    lib.check(lib.lib.mvlpt_op_layernorm_bwd_rows(E._TORCH2DT[F16], _ptr(dy_d), lib.DT_F32, _ptr(x_d), _ptr(g_d), _ptr(r_d), _ptr(r_d),
                                                  None, rows, d, 0, Lg, L, None), None, "layernorm_bwd_rows in place")
    assert _rel(r_d, ref) < 2e-5


# ------------------------------------------------------------------------------------------------ 1c: attention backward
def _attn_bwd64(qkv, dout, N, Ls, H):
    """Causal attention backward in float64 over full sequences: qkv [N * Ls, 3d], dout [N * Ls, d] -> dqkv [N * Ls, 3d]."""
    d = H * 64
    q, k, v = (t.reshape(N, Ls, H, 64).permute(0, 2, 1, 3) for t in qkv.double().reshape(N, Ls, 3 * d).split(d, dim=-1))
    do = dout.double().reshape(N, Ls, H, 64).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) / 8.0 + torch.full((Ls, Ls), float("-inf"), dtype=torch.float64).triu_(1)
    p = torch.softmax(s, -1)
    o = p @ v
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    dq, dk = ds @ k / 8.0, ds.transpose(-1, -2) @ q / 8.0
    return torch.cat([t.permute(0, 2, 1, 3).reshape(N * Ls, d) for t in (dq, dk, dv)], dim=-1)


def _compact(t, N, Lg, Ls):
    return t.reshape(N, Ls, -1)[:, :Lg].reshape(N * Lg, -1)


@pytest.mark.parametrize("Lg", LGS)
def test_pair_attention_backward_over_the_leading_positions(Lg):
    """dout is zero behind position Lg in the reference and absent on the device; qkv, O and lse are the saved full-length ones."""
    lib, E = _lib(), _E()
    N, H = CS, 2
    d = H * 64
    g = torch.Generator().manual_seed(300 + Lg)
    qkv = torch.randn(N * L, 3 * d, generator=g)
    dout = torch.randn(N * L, d, generator=g)
    dout.reshape(N, L, d)[:, Lg:] = 0.0
    qkv2 = E.split_pair(qkv, F16)
    ref = _compact(_attn_bwd64(E.join_pair(qkv2), dout, N, L, H), N, Lg, L)
    out2, lse = E.op_attention32_fwd_pair(qkv2.to(DEV), N, L, H, True)
    dout2 = E.split_pair(_compact(dout, N, Lg, L), F16).to(DEV)
    dqkv2 = torch.full((N * Lg, 6 * d), float("nan"), dtype=F16, device=DEV)
    delta = torch.empty(N * H * Lg, device=DEV)
    qkv2_d = qkv2.to(DEV)
    lib.check(lib.lib.mvlpt_op_attention_bwd_rows(E._TORCH2DT[F16], 1, 0, _ptr(qkv2_d), _ptr(out2), _ptr(dout2), _ptr(lse), _ptr(delta),
                                                  _ptr(dqkv2), N, Lg, L, H, None), None, "attention_bwd_rows pair")
    torch.cuda.synchronize()
    got = E.join_pair(dqkv2.cpu())
    for i, nm in enumerate("qkv"):
        e = _rel(got[:, i * d:(i + 1) * d], ref[:, i * d:(i + 1) * d])
        print(f"attn32 bwd rows Lg={Lg} d{nm}: {e:.2e}")
        assert e < 1e-5, f"d{nm}: {e}"                     # test_attention32_fwd_bwd


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("Lg", LGS)
def test_single_operand_attention_backward_over_the_leading_positions(Lg, dtype):
    lib, E = _lib(), _E()
    N, H = CS, 2
    d = H * 64
    g = torch.Generator().manual_seed(400 + Lg)
    qkv = torch.randn(N * L, 3 * d, generator=g).to(dtype)
    dout = torch.randn(N * L, d, generator=g).to(dtype)
    dout.reshape(N, L, d)[:, Lg:] = 0.0
    ref = _compact(_attn_bwd64(qkv, dout, N, L, H), N, Lg, L)
    qkv_d = qkv.to(DEV)
    out, lse = E.op_attention_fwd(qkv_d, N, L, H, True)
    dout_d = _compact(dout, N, Lg, L).contiguous().to(DEV)
    dqkv = torch.full((N * Lg, 3 * d), float("nan"), dtype=dtype, device=DEV)
    delta = torch.empty(N * H * Lg, device=DEV)
    lib.check(lib.lib.mvlpt_op_attention_bwd_rows(E._TORCH2DT[dtype], 0, 0, _ptr(qkv_d), _ptr(out), _ptr(dout_d), _ptr(lse), _ptr(delta),
                                                  _ptr(dqkv), N, Lg, L, H, None), None, "attention_bwd_rows single")
    torch.cuda.synchronize()
    for i, nm in enumerate("qkv"):
        e = _rel(dqkv[:, i * d:(i + 1) * d], ref[:, i * d:(i + 1) * d])
        print(f"attn bwd rows Lg={Lg} {dtype} d{nm}: {e:.2e}")
        assert e < TOL[dtype] * 3, f"d{nm}: {e}"            # test_attention_fwd_bwd


# ------------------------------------------------------------------------------------------------ 1d: context-gradient gather
@pytest.mark.parametrize("Lg", LGS)
def test_gather_ctx_grad_at_the_gradient_pitch(Lg):
    """The gather takes the compact gradient [C, Lg, d]: context positions up to Lg - 2 (an EOT at Lg - 1) and down to 1 (an EOT at 2)."""
    from mvlpt_amd.engine import op_gather_ctx_grad
    d, n = 128, 1
    g = torch.Generator().manual_seed(500 + Lg)
    dx = torch.randn(CS, Lg, d, generator=g)
    ctx_pos = torch.tensor([[Lg - 2], [1], [Lg // 2], [1], [2]], dtype=torch.int32)
    picked = dx[torch.arange(CS).view(CS, 1), ctx_pos.long()]
    a = op_gather_ctx_grad(dx.to(DEV), ctx_pos.to(DEV), False).cpu()
    assert _rel(a, picked.double().sum(0)) <= REDUCE_TOL
    assert torch.equal(op_gather_ctx_grad(dx.to(DEV), ctx_pos.to(DEV), True).cpu(), picked)


# ------------------------------------------------------------------------------------------------ 2: the tower, bit for bit
def _arch():
    from mvlpt_amd.weights import ClipArch
    # a two-block 128-wide image tower (never run here); text: 4 blocks of width 256 (LayerNorm folding needs 256), context 20
    return ClipArch("gradlen256", 128, 32, 2, 128, 16, L, 49408, 256, 4, 4)


class _Tower:
    def __init__(self, seed=31):
        from mvlpt_amd.model import FrozenCLIP, build_prompt_layout
        from mvlpt_amd.weights import make_state_dict
        self.arch = _arch()
        self.clip = FrozenCLIP(make_state_dict(self.arch, seed), device=DEV)
        self.eng = self.clip.engine
        g = torch.Generator().manual_seed(seed)
        dt, e, n = 256, self.arch.embed_dim, 1
        self.n, self.dt = n, dt
        self.layout = build_prompt_layout([1] * CS, n, L, "end").to(DEV)
        self.prefix = (torch.randn(CS, 1, dt, generator=g) * 0.02).to(DEV)
        self.suffix = (torch.randn(CS, L - 1 - n, dt, generator=g) * 0.02).to(DEV)
        self.ctx = (torch.randn(n, dt, generator=g) * 0.1).to(DEV)
        self.ctx_csc = (torch.randn(CS, n, dt, generator=g) * 0.1).to(DEV)
        self.ctx_deep = (torch.randn(2, n, dt, generator=g) * 0.1).to(DEV)
        self.ctx_grp = (torch.randn(3, n, dt, generator=g) * 0.1).to(DEV)
        self.dfeat = torch.randn(CS, e, generator=g).to(DEV)
        self.dfeat_r = torch.randn(5, e, generator=g).to(DEV)          # ranges [0,2) [2,2) [1,4): five sequences

    def eot(self, Lg):
        """EOT positions with the maximum Lg - 1 and the minimum 2 (the context token is at position 1)."""
        return torch.tensor([2, Lg - 1, min(4, Lg - 1), 2, Lg - 2], dtype=torch.int32, device=DEV)

    def run(self, kind, eot, grad_len):
        """(features, dctx[, dctx_deep]) of one saved step under the gradient length `grad_len`."""
        eng = self.eng
        eng.set_text_grad_len(grad_len, int(eot.max()))
        try:
            if kind == "deep":
                f = eng.text_fwd_deep(self.prefix, self.suffix, self.ctx, self.ctx_deep, self.layout, eot, save_for_bwd=True).clone()
                out = (f,) + tuple(t.clone() for t in eng.text_bwd_deep(self.dfeat))
            elif kind == "ranged":
                f = eng.text_fwd_ranged(self.prefix, self.suffix, self.ctx_grp, self.layout, eot, [0, 2, 1], [2, 2, 4], save_for_bwd=True).clone()
                out = (f, eng.text_bwd(self.dfeat_r).clone())
            else:
                f = eng.text_fwd(self.prefix, self.suffix, self.ctx_csc if kind == "csc" else self.ctx, self.layout, eot, save_for_bwd=True).clone()
                out = (f, eng.text_bwd(self.dfeat).clone())
            torch.cuda.synchronize()
        finally:
            eng.set_text_grad_len(L, 0)
        return out


@pytest.fixture(scope="module")
def tower():
    return _Tower()


def _assert_same_bits(tower, kind, Lg, what):
    eot = tower.eot(Lg)
    full, short = tower.run(kind, eot, L), tower.run(kind, eot, Lg)
    assert all(bool(t.abs().max() > 0) for t in full[1:]), f"{what}: a zero gradient proves nothing"
    for a, b, nm in zip(full, short, ("features", "dctx", "dctx_deep")):
        assert torch.equal(a, b), f"{what} Lg={Lg}: {nm} differs from Lg = L by {float((a - b).abs().max()):.3e} (max|ref| {float(a.abs().max()):.3e})"


@pytest.mark.parametrize("Lg", [7, 16, 17])
@pytest.mark.parametrize("kind", ["plain", "csc", "deep", "ranged"])
def test_tower_gradients_keep_their_bits(tower, kind, Lg):
    """Plain, class-specific, deep (n_deep = 2) and ranged (one empty range) towers in the engine's default mode."""
    _assert_same_bits(tower, kind, Lg, kind)


@pytest.mark.parametrize("mode", ["split_grad", "split_all", "fast"])
@pytest.mark.parametrize("fold", [0, 2])
def test_tower_gradients_keep_their_bits_in_every_mode(tower, mode, fold):
    """Both gradient precisions (and the 16-bit-pair mode), LayerNorm folding forced on (threshold of one row) and off."""
    eng = tower.eng
    eng.set_precision(mode)
    eng.set_ln_fold(fold, 1)
    try:
        for kind in ("plain", "deep"):
            _assert_same_bits(tower, kind, 7, f"{mode} fold={fold} {kind}")
    finally:
        eng.set_precision("split_grad")
        eng.set_ln_fold(2)


@pytest.mark.parametrize("kind", ["plain", "deep", "ranged"])
def test_tower_gradients_keep_their_bits_under_activation_checkpointing(tower, kind):
    tower.eng.set_text_act_ckpt(2)
    try:
        _assert_same_bits(tower, kind, 7, f"ACT_CKPT=2 {kind}")
    finally:
        tower.eng.set_text_act_ckpt(1)


@pytest.mark.parametrize("mode", ["split_grad", "fast"])
def test_tower_keeps_its_bits_where_the_row_count_changes_the_kernels(mode):
    """100 classes of 77 positions, width 512, max(eot) = 23: 7 700 saved rows take the grid-stride LayerNorm and the GEMM routes of
    many tiles, the 2 400 gradient rows alone would take the one-wave LayerNorm and other GEMM routes.  Three blocks suffice."""
    from mvlpt_amd.model import FrozenCLIP, build_prompt_layout
    from mvlpt_amd.weights import ClipArch, make_state_dict
    C_, Ls, Lg, d, n = 100, 77, 24, 512, 16
    arch = ClipArch("gradlen512", 128, 32, 2, 128, 16, Ls, 49408, d, d // 64, 3)
    eng = FrozenCLIP(make_state_dict(arch, 34), device=DEV, precision=mode).engine
    g = torch.Generator().manual_seed(34)
    layout = build_prompt_layout([1] * C_, n, Ls, "end").to(DEV)
    eot = torch.tensor([n + 2 + c % 6 for c in range(C_)], dtype=torch.int32, device=DEV)          # 18 .. 23
    prefix = (torch.randn(C_, 1, d, generator=g) * 0.02).to(DEV)
    suffix = (torch.randn(C_, Ls - 1 - n, d, generator=g) * 0.02).to(DEV)
    ctx = (torch.randn(n, d, generator=g) * 0.1).to(DEV)
    dfeat = torch.randn(C_, arch.embed_dim, generator=g).to(DEV)
    res = {}
    for grad_len in (Ls, Lg):
        eng.set_text_grad_len(grad_len, Lg - 1)
        eng.text_fwd(prefix, suffix, ctx, layout, eot, save_for_bwd=True)
        res[grad_len] = eng.text_bwd(dfeat).clone()
    torch.cuda.synchronize()
    a, b = res[Ls], res[Lg]
    assert bool(a.abs().max() > 0)
    assert torch.equal(a, b), f"{mode}: dctx differs by {float((a - b).abs().max()):.3e} (max|ref| {float(a.abs().max()):.3e})"


def test_exact_gelu_tower_keeps_its_bits():
    """The stand-alone activation pass reads the saved pre-activation through the same map."""
    t = _Tower(seed=32)
    t.eng.set_activation("gelu")
    _assert_same_bits(t, "plain", 7, "exact GELU")


# ------------------------------------------------------------------------------------------------ 3: arguments and state
def test_setter_and_forward_refuse_bad_lengths(tower):
    lib, eng = _lib(), tower.eng
    for bad in (2, 0, -1, L + 1):
        assert lib.lib.mvlpt_set_text_grad_len(eng.h, bad, 5) == lib.ERR_ARG and "set_text_grad_len" in lib.last_error(eng.h), bad
    assert lib.lib.mvlpt_set_text_grad_len(eng.h, 7, -1) == lib.ERR_ARG
    with pytest.raises(RuntimeError):
        eng.set_text_grad_len(L + 1, 5)
    eot = tower.eot(7)                                    # max(eot) = 6
    feat = torch.full((CS, tower.arch.embed_dim), 7.0, device=DEV)
    job = lib.MvlptTextJob(prefix=tower.prefix.data_ptr(), suffix=tower.suffix.data_ptr(), ctx=tower.ctx.data_ptr(), n_ctx=tower.n,
                           layout=tower.layout.data_ptr(), eot=eot.data_ptr(), n_cls=CS, L=L, save_for_bwd=1)
    try:
        for grad_len in (6, 5, 3):                        # does not reach the largest EOT position
            eng.set_text_grad_len(grad_len, 6)
            with torch.cuda.device(eng.device):
                rc = lib.lib.mvlpt_text_fwd(eng.h, C.byref(job), _ptr(feat), None)
            torch.cuda.synchronize()
            assert rc == lib.ERR_ARG and "gradient length" in lib.last_error(eng.h), grad_len
            assert bool((feat == 7.0).all()), "a refused forward must not launch"
            with pytest.raises(RuntimeError):
                eng.text_fwd_deep(tower.prefix, tower.suffix, tower.ctx, tower.ctx_deep, tower.layout, eot, save_for_bwd=True)
            with pytest.raises(RuntimeError):
                eng.text_fwd_ranged(tower.prefix, tower.suffix, tower.ctx_grp, tower.layout, eot, [0, 2, 1], [2, 2, 4], save_for_bwd=True)
            # a forward that saves nothing has no backward to shorten
            f = eng.text_fwd(tower.prefix, tower.suffix, tower.ctx, tower.layout, eot, save_for_bwd=False)
            assert bool(torch.isfinite(f).all())
    finally:
        eng.set_text_grad_len(L, 0)


def test_a_forward_records_its_own_gradient_length(tower):
    """A call between a forward and its backward changes nothing, in either direction."""
    eng, eot = tower.eng, tower.eot(7)
    _, want = tower.run("plain", eot, L)
    try:
        for at_fwd, at_bwd in ((7, L), (L, 7), (7, 16)):
            eng.set_text_grad_len(at_fwd, 6)
            eng.text_fwd(tower.prefix, tower.suffix, tower.ctx, tower.layout, eot, save_for_bwd=True)
            eng.set_text_grad_len(at_bwd, 6)
            d = eng.text_bwd(tower.dfeat).clone()
            assert torch.equal(d, want), (at_fwd, at_bwd)
            assert torch.equal(eng.text_bwd(tower.dfeat), want), "a second backward on the same saved state"
    finally:
        eng.set_text_grad_len(L, 0)


def _launches(tower, eot, setting):
    eng = tower.eng
    if setting is not None:
        eng.set_text_grad_len(*setting)
    eng.profile_begin(all_kernels=True)
    eng.text_fwd(tower.prefix, tower.suffix, tower.ctx, tower.layout, eot, save_for_bwd=True)
    eng.text_bwd(tower.dfeat)
    torch.cuda.synchronize()
    return {k: v["launches"] for k, v in eng.profile_end().items()}


def test_default_length_launches_what_an_untouched_engine_launches():
    """An engine whose setter was never called and one set to the full length enqueue the same kernels on the same shapes (the GEMM
    records carry M x N x K).  One set to max(eot) + 1 enqueues as many, class by class: the gradient length changes the M of the
    backward's GEMMs, never the list of launches."""
    t = _Tower(seed=33)
    eot = t.eot(7)
    try:
        fresh = _launches(t, eot, None)
        full = _launches(t, eot, (L, 6))
        short = _launches(t, eot, (7, 6))
    finally:
        t.eng.set_text_grad_len(L, 0)
    assert sum(fresh.values()) > 0 and fresh == full, (fresh, full)

    def by_class(stats):      # "g<M>x<N>x<K> e<epi> s<split> f<fold>" -> the record without its M
        out = {}
        for k, v in stats.items():
            key = "g" + k.split("x", 1)[1] if k.startswith("g") and "x" in k else k
            out[key] = out.get(key, 0) + v
        return out
    assert by_class(short) == by_class(fresh), (fresh, short)
    assert any(k.startswith(f"g{CS * 7}x") for k in short) and not any(k.startswith(f"g{CS * 7}x") for k in fresh), short


def test_models_set_the_length_of_their_class_table():
    """CustomCLIP tells the engine max(eot) + 1 in front of a saving forward; TEXT_GRAD_TO_EOT = False restores the full length; the
    prompt gradient has the same bits either way."""
    import tests.test_hip_model as M
    from mvlpt_amd.model import FrozenCLIP
    from tests.golden_util import load_npz, t, tiny_state_dict
    case = load_npz("tiny_coop_cut")
    clip = FrozenCLIP(tiny_state_dict(), compute_dtype="fp16")
    seen, grads = [], {}
    setter = clip.engine.set_text_grad_len
    clip.engine.set_text_grad_len = lambda grad_len, max_eot: (seen.append((grad_len, max_eot)), setter(grad_len, max_eot))[1]
    for on in (True, False):
        model = M.build_model(case, clip, 32, t(case["token_prefix"]), t(case["token_suffix"]))
        assert model.text_grad_to_eot is True
        model.text_grad_to_eot = on
        model.prompt_learner.zero_grad(set_to_none=True)
        logits = model(t(case["image"]).to(clip.device), task=None)
        model.cross_entropy(logits, t(case["label"]).to(clip.device)).backward()
        torch.cuda.synchronize()
        grads[on] = model.prompt_learner.ctx.grad.clone()
        m = model.prompt_learner.max_eot
        assert seen[-1] == ((m + 1, m) if on else (clip.context_length, m)), seen
    assert torch.equal(grads[True], grads[False]) and bool(grads[True].abs().max() > 0)
