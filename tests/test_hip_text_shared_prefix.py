"""Shared prefix of the text tower (-m gpu): mvlpt_set_text_shared_prefix / TRAINER.MVLPT.TEXT_SHARED_PREFIX.

With a generic context the first P positions of every class prompt are the same rows, the attention is causal and everything else acts
row by row: the tower evaluates them once.  Rows live in C + 1 slots (slot 0: the prefix in its first P rows, slot c + 1: positions
P .. of class c); the backward carries the prefix gradient summed over the classes, and dK / dV of the prefix keys go through fp32
partials and a reduction in a fixed order.

1. kernel level: the pair attention forward, backward and reduction in the slot layout against a float64 restatement in this file
   (the prefix expanded to every sequence, its gradient summed over the sequences), at the bounds tests/test_hip_ops.py and
   tests/test_hip_text_bwd_rows.py apply to the same kernels; rows that must not be read hold NaN, the unused rows of slot 0 come out
   as zeros; mixed pairs against 16-bit pairs as tests/test_hip_mixed_pair.py compares them;
2. tower level: features with the bits of P = 0, dctx of the positions behind the prefix with the bits of P = 0, dctx of the prefix
   positions against the CPU oracle inside the bound of the parity tests, for both settings;
3. arguments, fallback routes and state."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
H, D = 2, 128                                   # two heads of 64
O_TOL, LSE_TOL, BWD_TOL = 5e-6, 1e-5, 1e-5      # tests/test_hip_ops.py test_attention32_fwd_bwd; test_hip_text_bwd_rows.py
DCTX_TOL = 1e-3                                 # the parity tests' bound on dctx, of max |dctx| (tests/test_hip_model.py GRAD_TOL_FP16)
# ... and their bf16 bound (GRAD_TOL_BF16: bf16 MFMA inputs round the frozen weights to 8 bits; the tower WITHOUT a prefix is at
# 7e-3 of max |dctx| here).  The two settings differ by a summation order in fp32 and one pair rounding of the summed gradient per
# block, so P > 0 is also held to DCTX_TOL against P = 0 in both types.
ORACLE_TOL = {"fp16": DCTX_TOL, "bf16": 6e-2}
# MVLPT_PREC_FAST (single 16-bit operands everywhere) is a secondary mode with its own parity bound on gradients, GRAD_TOL_FAST = 5e-3
# (tests/test_hip_model.py).  There the shared prefix rounds the class SUM of a prefix gradient to 16 bits where P = 0 rounds every
# class's term, several times per block: two fast-mode evaluations of one gradient, each inside that bound of the truth, are held to
# the same bound against each other.
FAST_TOL = {"fp16": 5e-3, "bf16": 6e-2}
SHAPES = [(20, 20, 1), (20, 11, 4), (20, 20, 9), (40, 33, 16), (40, 40, 17)]      # (L, Lg, P): P below, on and across a 16-row tile edge


def _rel(a, b):
    """max |a - b| / max |b|; a reference that is zero (dQ / dK of a one-position prefix: softmax over one key) counts as scale 1,
    as in tests/test_hip_ops.py test_attention32_fwd_bwd"""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / (scale if scale >= 1e-6 else 1.0)


def _lib():
    from mvlpt_amd import _lib
    return _lib


def _E():
    from mvlpt_amd import engine
    return engine


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ 1: kernels against float64
def _heads(t, N, L):
    return t.reshape(N, L, H, 64).permute(0, 2, 1, 3)


def _attn64(qkv, N, L):
    """Causal attention over full sequences in float64: qkv [N, L, 3d] -> (q, k, v, p, o [N, H, L, 64], lse [N, H, L])."""
    q, k, v = (_heads(t, N, L) for t in qkv.double().split(D, dim=-1))
    s = q @ k.transpose(-1, -2) / 8.0 + torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    p = torch.softmax(s, -1)
    return q, k, v, p, p @ v, torch.logsumexp(s, -1)


def _attn_bwd64(qkv, dout, N, L):
    """-> dqkv [N, L, 3d]"""
    q, k, v, p, o, _ = _attn64(qkv, N, L)
    do = _heads(dout.double(), N, L)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    dq, dk = ds @ k / 8.0, ds.transpose(-1, -2) @ q / 8.0
    return torch.cat([t.permute(0, 2, 1, 3).reshape(N, L, D) for t in (dq, dk, dv)], dim=-1)


def _slots(pre, cls, rows, fill):
    """[(N + 1) * rows, w]: slot 0 = `pre` [P, w] then `fill`, slot n + 1 = cls[n] [rows, w]"""
    N, w = cls.shape[0], cls.shape[-1]
    out = torch.full((N + 1, rows, w), fill, dtype=cls.dtype)
    out[0, :pre.shape[0]] = pre
    out[1:] = cls
    return out.reshape((N + 1) * rows, w)


class _Case:
    """One (N, L, Lg, P): inputs in the slot layout on the device, the expanded float64 problem on the host."""

    def __init__(self, N, L, Lg, P):
        E = _E()
        self.N, self.L, self.Lg, self.P, self.Lf, self.Lt = N, L, Lg, P, L - P, Lg - P
        g = torch.Generator().manual_seed(7000 + 100 * L + 10 * P + N)
        nan = float("nan")
        # what the kernels read: 16-bit pairs; the reference takes the values the pairs hold
        pre2 = E.split_pair(torch.randn(P, 3 * D, generator=g), F16)
        cls2 = E.split_pair(torch.randn(N * self.Lf, 3 * D, generator=g), F16)
        self.qkv_slots = _slots(pre2, cls2.reshape(N, self.Lf, 6 * D), self.Lf, nan).to(DEV)
        pre, cls = E.join_pair(pre2), E.join_pair(cls2).reshape(N, self.Lf, 3 * D)
        self.qkv = torch.cat([pre.unsqueeze(0).expand(N, P, 3 * D), cls], dim=1)          # the prefix expanded: [N, L, 3d]
        # gradients: positions P .. Lg-1 of every class, and the prefix's own (the sum the row-wise kernels hand it)
        g0 = E.split_pair(torch.randn(P, D, generator=g), F16)
        gc = E.split_pair(torch.randn(N * self.Lt, D, generator=g), F16)
        self.dout_slots = _slots(g0, gc.reshape(N, self.Lt, 2 * D), self.Lt, nan).to(DEV)
        self.d_own = torch.zeros(N, L, D)
        self.d_own[0, :P] = E.join_pair(g0)                       # expanded: attributed to sequence 0 (O[:P] is the same in all)
        self.d_cls = torch.zeros(N, L, D)
        self.d_cls[:, P:Lg] = E.join_pair(gc).reshape(N, self.Lt, D)

    def forward(self, lo8=0):
        lib, E = _lib(), _E()
        out = torch.full(((self.N + 1) * self.Lf, 2 * D), float("nan"), dtype=F16, device=DEV)
        lse = torch.full((self.N + 1, H, self.Lf), float("nan"), device=DEV)
        lib.check(lib.lib.mvlpt_op_attention32_fwd_prefix(E._TORCH2DT[F16], lo8, _ptr(self.qkv_slots), _ptr(out), _ptr(lse), self.N, self.L, H,
                                                          self.P, None), None, "attention32_fwd_prefix")
        torch.cuda.synchronize()
        return out, lse

    def backward(self, out, lse, mul=1.0, lo8=0):
        lib, E = _lib(), _E()
        dqkv = torch.full(((self.N + 1) * self.Lt, 6 * D), float("nan"), dtype=F16, device=DEV)
        part = torch.full((self.N + 1, self.P, 2 * D), float("nan"), device=DEV)
        delta = torch.empty((self.N + 1) * H * self.Lg, device=DEV)
        lib.check(lib.lib.mvlpt_op_attention32_bwd_prefix(E._TORCH2DT[F16], lo8, _ptr(self.qkv_slots), _ptr(out), _ptr(self.dout_slots), _ptr(lse),
                                                          _ptr(delta), _ptr(dqkv), _ptr(part), C.c_float(mul), self.N, self.Lg, self.L, H,
                                                          self.P, None), None, "attention32_bwd_prefix")
        torch.cuda.synchronize()
        return dqkv, part


@pytest.mark.parametrize("N", [1, 5, 37])
@pytest.mark.parametrize("L,Lg,P", SHAPES)
def test_pair_attention_in_the_slot_layout(L, Lg, P, N):
    E = _E()
    c = _Case(N, L, Lg, P)
    Lf, Lt = c.Lf, c.Lt
    # ---- forward
    out, lse = c.forward()
    _, _, _, _, o64, lse64 = _attn64(c.qkv, N, L)
    o64 = o64.permute(0, 2, 1, 3).reshape(N, L, D)
    got_o = E.join_pair(out.cpu()).reshape(N + 1, Lf, D)
    got_lse = lse.cpu()
    # the unused rows of slot 0: zeros (finite, deterministic contents for the row-wise kernels behind the attention), never results
    assert float(out.cpu().reshape(N + 1, Lf, 2 * D)[0, P:].float().abs().max()) == 0.0, "the unused rows of slot 0 of O hold zeros"
    assert float(got_lse[0, :, P:].abs().max()) == 0.0, "lse of the unused rows of slot 0 holds zeros"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), "a NaN row was read, or a row was not written"
    e_cls, e_pre = _rel(got_o[1:], o64[:, P:]), _rel(got_o[0, :P], o64[0, :P])
    e_lse = max(float((got_lse[1:] - lse64[:, :, P:]).abs().max()), float((got_lse[0, :, :P] - lse64[0, :, :P]).abs().max()))
    print(f"fwd N={N} L={L} P={P}: O class slots {e_cls:.2e}, prefix {e_pre:.2e}, lse {e_lse:.2e}")
    assert e_cls < O_TOL and e_pre < O_TOL and e_lse < LSE_TOL, (e_cls, e_pre, e_lse)
    # ---- backward + reduction, the class partials entering at 1 and (one case) at 1/2
    own, cls = _attn_bwd64(c.qkv, c.d_own, N, L), _attn_bwd64(c.qkv, c.d_cls, N, L)
    assert float(cls[:, :P, :D].abs().max()) == 0.0          # no dO on a class's prefix queries: dQ there is the prefix's own
    for mul in ((1.0, 0.5) if (N, P) == (5, 4) else (1.0,)):
        dqkv, part = c.backward(out, lse, mul)
        assert bool(torch.isfinite(part).all()), "a partial was not written"
        got = E.join_pair(dqkv.cpu()).reshape(N + 1, Lt, 3 * D)
        assert bool(torch.isfinite(got).all()), "a NaN row was read, or a gradient row was not written"
        assert float(got[0, P:].abs().max()) == 0.0 if Lt > P else True, "the unused rows of slot 0 are written as zeros"
        want0 = own[0, :P].clone()
        want0[:, D:] += mul * cls[:, :P, D:].sum(0)
        for i, nm in enumerate("qkv"):
            sl = slice(i * D, (i + 1) * D)
            e1, e0 = _rel(got[1:, :, sl], cls[:, P:Lg, sl]), _rel(got[0, :P, sl], want0[:, sl])
            print(f"bwd N={N} L={L} Lg={Lg} P={P} mul={mul} d{nm}: class slots {e1:.2e}, slot 0 {e0:.2e}")
            assert e1 < BWD_TOL and e0 < BWD_TOL, f"d{nm}: {e1} {e0}"
        # the same launches again: the same bits (a fixed summation order, no atomics)
        again, _ = c.backward(out, lse, mul)
        assert torch.equal(again.view(torch.int16), dqkv.view(torch.int16))


@pytest.mark.parametrize("L,Lg,P", [(20, 11, 4), (40, 40, 17)])
def test_mixed_pair_outputs_in_the_slot_layout(L, Lg, P):
    """O and dQ | dK | dV written as mixed pairs (hi plane + e5m2 residual bytes), delta read from a mixed O, the reduction's stores
    included: the hi planes of the 16-bit-pair run, values to the mixed pair's own resolution (tests/test_hip_mixed_pair.py)."""
    from tests.test_hip_mixed_pair import PAIR_TOL
    E = _E()
    c = _Case(5, L, Lg, P)
    o_pair, lse = c.forward()
    o_mix, lse_m = c.forward(lo8=1)
    assert torch.equal(lse, lse_m) and torch.equal(o_pair[:, :D], o_mix[:, :D])
    assert _rel(E.join_mixed(o_mix.cpu()), E.join_pair(o_pair.cpu())) < PAIR_TOL[F16]
    ref = E.join_pair(c.backward(o_pair, lse)[0].cpu())
    got = E.join_mixed(c.backward(o_mix, lse, lo8=1)[0].cpu())
    assert bool(torch.isfinite(got).all())
    slot0 = slice(0, P)
    for i, nm in enumerate("qkv"):
        sl = slice(i * D, (i + 1) * D)
        e1, e0 = _rel(got[c.Lt:, sl], ref[c.Lt:, sl]), _rel(got[slot0, sl], ref[slot0, sl])
        print(f"mixed L={L} Lg={Lg} P={P} d{nm}: class slots {e1:.2e}, slot 0 {e0:.2e}")
        assert e1 < 3 * PAIR_TOL[F16] and e0 < 3 * PAIR_TOL[F16], f"d{nm}: {e1} {e0}"
    assert float(got[P:c.Lt].abs().max()) == 0.0


TOL16 = {F16: 2e-3, BF16: 1.6e-2}      # tests/test_hip_ops.py: output rounding of the 16-bit type (backward: 3 x, test_attention_fwd_bwd)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("N", [1, 5, 37])
@pytest.mark.parametrize("L,Lg,P", SHAPES)
def test_single_operand_attention_in_the_slot_layout(L, Lg, P, N, dtype):
    """The fast mode's kernels (attention.hip) in the same layout: forward, dQ, dK / dV and the reduction against float64, at the
    bounds tests/test_hip_text_bwd_rows.py applies to them; NaN in every row that must not be read, zeros in slot 0's unused rows."""
    lib, E = _lib(), _E()
    Lf, Lt, dt = L - P, Lg - P, E._TORCH2DT[dtype]
    g = torch.Generator().manual_seed(9000 + 100 * L + 10 * P + N)
    nan = float("nan")
    pre = torch.randn(P, 3 * D, generator=g).to(dtype)
    cls = torch.randn(N, Lf, 3 * D, generator=g).to(dtype)
    qkv_slots = _slots(pre, cls, Lf, nan).to(DEV)
    qkv = torch.cat([pre.unsqueeze(0).expand(N, P, 3 * D), cls], dim=1).float()
    out = torch.full(((N + 1) * Lf, D), nan, dtype=dtype, device=DEV)
    lse = torch.full((N + 1, H, Lf), nan, device=DEV)
    lib.check(lib.lib.mvlpt_op_attention_fwd_prefix(dt, _ptr(qkv_slots), _ptr(out), _ptr(lse), N, L, H, P, None), None, "attention_fwd_prefix")
    torch.cuda.synchronize()
    _, _, _, _, o64, lse64 = _attn64(qkv, N, L)
    o64 = o64.permute(0, 2, 1, 3).reshape(N, L, D)
    got_o, got_lse = out.cpu().float().reshape(N + 1, Lf, D), lse.cpu()
    assert bool(torch.isfinite(got_o).all()) and bool(torch.isfinite(got_lse).all())
    assert float(got_o[0, P:].abs().max() if Lf > P else 0.0) == 0.0 and float(got_lse[0, :, P:].abs().max() if Lf > P else 0.0) == 0.0
    e_cls, e_pre = _rel(got_o[1:], o64[:, P:]), _rel(got_o[0, :P], o64[0, :P])
    e_lse = max(float((got_lse[1:] - lse64[:, :, P:]).abs().max()), float((got_lse[0, :, :P] - lse64[0, :, :P]).abs().max()))
    print(f"single fwd {dtype} N={N} L={L} P={P}: O class slots {e_cls:.2e}, prefix {e_pre:.2e}, lse {e_lse:.2e}")
    assert e_cls < TOL16[dtype] and e_pre < TOL16[dtype] and e_lse < 1e-5 * (1 if dtype == F16 else 8), (e_cls, e_pre, e_lse)
    # backward
    g0 = torch.randn(P, D, generator=g).to(dtype)
    gc = torch.randn(N, Lt, D, generator=g).to(dtype)
    dout_slots = _slots(g0, gc, Lt, nan).to(DEV)
    d_own, d_cls = torch.zeros(N, L, D), torch.zeros(N, L, D)
    d_own[0, :P], d_cls[:, P:Lg] = g0.float(), gc.float()
    own, cl = _attn_bwd64(qkv, d_own, N, L), _attn_bwd64(qkv, d_cls, N, L)
    for mul in ((1.0, 0.5) if (N, P) == (5, 4) else (1.0,)):
        dqkv = torch.full(((N + 1) * Lt, 3 * D), nan, dtype=dtype, device=DEV)
        part = torch.full((N + 1, P, 2 * D), nan, device=DEV)
        delta = torch.full(((N + 1) * H * Lt,), nan, device=DEV)
        lib.check(lib.lib.mvlpt_op_attention_bwd_prefix(dt, _ptr(qkv_slots), _ptr(out), _ptr(dout_slots), _ptr(lse), _ptr(delta), _ptr(dqkv),
                                                        _ptr(part), C.c_float(mul), N, Lg, L, H, P, None), None, "attention_bwd_prefix")
        torch.cuda.synchronize()
        got = dqkv.cpu().float().reshape(N + 1, Lt, 3 * D)
        bad = (~torch.isfinite(got)).nonzero()
        assert bool(torch.isfinite(part).all()) and bad.numel() == 0, \
            f"not finite: {bad.shape[0]} entries, slots {bad[:, 0].unique().tolist()} rows {bad[:, 1].unique().tolist()} " \
            f"columns {int(bad[:, 2].min())} .. {int(bad[:, 2].max())}"
        assert float(got[0, P:].abs().max() if Lt > P else 0.0) == 0.0
        want0 = own[0, :P].clone()
        want0[:, D:] += mul * cl[:, :P, D:].sum(0)
        for i, nm in enumerate("qkv"):
            sl = slice(i * D, (i + 1) * D)
            e1, e0 = _rel(got[1:, :, sl], cl[:, P:Lg, sl]), _rel(got[0, :P, sl], want0[:, sl])
            print(f"single bwd {dtype} N={N} L={L} Lg={Lg} P={P} mul={mul} d{nm}: class slots {e1:.2e}, slot 0 {e0:.2e}")
            assert e1 < 3 * TOL16[dtype] and e0 < 3 * TOL16[dtype], f"d{nm}: {e1} {e0}"


def test_prefix_kernels_check_their_arguments():
    lib, E = _lib(), _E()
    t = torch.zeros(64 * 1024, dtype=torch.float32, device=DEV)
    dt = E._TORCH2DT[F16]
    for L, P in ((20, 0), (20, -1), (20, 20), (20, 11), (81, 4)):      # no prefix, negative, the whole sequence, more than slot 0 holds, too long
        assert lib.lib.mvlpt_op_attention32_fwd_prefix(dt, 0, _ptr(t), _ptr(t), _ptr(t), 2, L, H, P, None) != 0, (L, P)
    for Lg, Ls, P in ((20, 20, 0), (20, 20, 11), (20, 12, 4), (81, 81, 4)):    # ..., a prefix that does not fit a gradient slot, Ls < Lg
        assert lib.lib.mvlpt_op_attention32_bwd_prefix(dt, 0, _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), C.c_float(1.0),
                                                       2, Lg, Ls, H, P, None) != 0, (Lg, Ls, P)
    assert lib.lib.mvlpt_op_attention32_bwd_prefix(dt, 0, _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), _ptr(t), None, C.c_float(1.0),
                                                   2, 20, 20, H, 4, None) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2: the tower
N_CTX = 6


def _arch(L):
    from mvlpt_amd.weights import ClipArch
    # the `tiny` text tower (width 128, 2 heads, 2 blocks) at a short context; the image tower is never run here
    return ClipArch(f"tinyprefix{L}", 128, 32, 2, 128, 16, L, 49408, 128, 2, 2)


class _Tower:
    """C classes, "middle": SOS + 3 context rows in front of the class name (P = 4), 3 behind it."""

    def __init__(self, C_, L, mode="split_grad", dtype="fp16", seed=41, position="middle"):
        from mvlpt_amd.model import FrozenCLIP, build_prompt_layout
        from mvlpt_amd.weights import make_state_dict
        from tests.fake_engine import OracleEngine
        self.C, self.L, self.arch = C_, L, _arch(L)
        self.sd = make_state_dict(self.arch, seed)
        self.clip = FrozenCLIP(self.sd, compute_dtype=dtype, device=DEV, precision=mode)      # (kept: it owns the token table's loader)
        self.eng = self.clip.engine
        self.oracle = OracleEngine(self.sd, self.arch)
        g = torch.Generator().manual_seed(seed)
        n, dt = N_CTX, 128
        lens = [1 + c % 3 for c in range(C_)]                                   # class names of 1 .. 3 tokens
        self.layout = build_prompt_layout(lens, n, L, position)
        self.P_layout = 1 + (n // 2 if position == "middle" else n if position == "end" else 0)
        self.eot = torch.tensor([1 + n + ln + 1 for ln in lens], dtype=torch.int32)      # SOS, ctx, name, '.', EOT
        row = torch.randn(1, 1, dt, generator=g) * 0.02
        self.prefix = row.expand(C_, 1, dt).contiguous()                        # one SOS embedding
        self.suffix = torch.randn(C_, L - 1 - n, dt, generator=g) * 0.02
        self.ctx = torch.randn(n, dt, generator=g) * 0.1
        self.dfeat = torch.randn(C_, self.arch.embed_dim, generator=g)
        self.dev = {k: getattr(self, k).to(DEV) for k in ("layout", "eot", "prefix", "suffix", "ctx", "dfeat")}
        self.max_eot = int(self.eot.max())

    def run(self, P, grad_len=None):
        eng, d = self.eng, self.dev
        eng.set_text_grad_len(grad_len or self.L, self.max_eot)
        eng.set_text_shared_prefix(P)
        try:
            f = eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=True).clone()
            g = eng.text_bwd(d["dfeat"]).clone()
            torch.cuda.synchronize()
        finally:
            eng.set_text_shared_prefix(0)
            eng.set_text_grad_len(self.L, 0)
        return f, g

    def reference(self):
        if not hasattr(self, "_ref"):
            f = self.oracle.text_fwd(self.prefix, self.suffix, self.ctx, self.layout, self.eot, save_for_bwd=True)
            self._ref = (f, self.oracle.text_bwd(self.dfeat))
        return self._ref

    def ctx_rows(self, P):
        """context rows whose position lies inside / behind the prefix (the same in every class for the rows inside)"""
        pos = {int(-e - 1): p for p, e in enumerate(self.layout[0].tolist()) if e < 0}
        inside = [j for j in range(N_CTX) if pos[j] < P]
        return inside, [j for j in range(N_CTX) if j not in inside]


_TOWERS = {}


def _tower(C_, L, mode, dtype):
    key = (C_, L, mode, dtype)
    if key not in _TOWERS:
        _TOWERS[key] = _Tower(C_, L, mode, dtype)
    return _TOWERS[key]


def _check_tower(t, P, grad_len, what, dtype="fp16"):
    f0, g0 = t.run(0, grad_len)
    f1, g1 = t.run(P, grad_len)
    fr, gr = t.reference()
    assert bool(g0.abs().max() > 0)
    assert torch.equal(f0, f1), f"{what}: features differ by {float((f0 - f1).abs().max()):.3e}"
    inside, behind = t.ctx_rows(P)
    assert inside and behind, "the case must have context rows on both sides of the prefix"
    assert torch.equal(g0[behind], g1[behind]), \
        f"{what}: dctx behind the prefix differs by {float((g0[behind] - g1[behind]).abs().max()):.3e}"
    scale = float(gr.abs().max())
    e0, e1 = float((g0.cpu() - gr).abs().max()) / scale, float((g1.cpu() - gr).abs().max()) / scale
    ei = float((g1[inside].cpu() - gr[inside]).abs().max()) / scale
    ed = float((g1[inside] - g0[inside]).abs().max()) / scale
    print(f"{what} P={P} Lg={grad_len}: dctx against the CPU oracle: P=0 {e0:.2e}, shared prefix {e1:.2e} (prefix rows {ei:.2e}); "
          f"prefix rows P>0 against P=0: {ed:.2e}")
    fast = "fast" in what
    tol = FAST_TOL[dtype] if fast else ORACLE_TOL[dtype]
    assert e0 < tol and e1 < tol and ed < (FAST_TOL[dtype] if fast else DCTX_TOL), (e0, e1, ed)
    # two runs: the same bits
    f2, g2 = t.run(P, grad_len)
    assert torch.equal(f1, f2) and torch.equal(g1, g2), f"{what}: a second run gives other bits"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", ["split_grad", "split_all", "fast"])
@pytest.mark.parametrize("C_", [5, 37])
def test_tower_with_a_shared_prefix(C_, mode, dtype):
    """Split operands (mixed pairs / 16-bit pairs) and single operands (fast: the kernels of attention.hip), both 16-bit types,
    Lg = L and Lg = max(eot) + 1."""
    t = _tower(C_, 20, mode, dtype)
    for grad_len in (t.L, t.max_eot + 1):
        _check_tower(t, t.P_layout, grad_len, f"C={C_} {mode} {dtype}", dtype)


def test_tower_with_a_prefix_shorter_than_the_layout_offers():
    """Any shorter prefix is as correct: P = 1 (SOS alone) and P = 2 on the same tower."""
    t = _tower(5, 20, "split_grad", "fp16")
    f0, g0 = t.run(0)
    for P in (1, 2):
        f1, g1 = t.run(P)
        _, behind = t.ctx_rows(P)
        assert torch.equal(f0, f1) and torch.equal(g0[behind], g1[behind]), P
        assert _rel(g1, g0) < DCTX_TOL


def test_many_classes_scale_the_prefix_gradient():
    """600 classes: the class partials enter slot 0 at 1/2 and the gather undoes it."""
    t = _tower(600, 12, "split_grad", "fp16")
    assert t.P_layout == 4
    _check_tower(t, 4, t.L, "C=600")


def test_fast_mode_shares_too():
    """Single operands run the slot layout as well: the GEMMs see (C + 1) (L - P) rows, and 600 classes scale the prefix gradient."""
    t = _tower(5, 20, "fast", "fp16")
    on = _launches(t, t.P_layout)
    assert any(k.startswith(f"g{6 * (20 - t.P_layout)}x") for k in on) and not any(k.startswith(f"g{5 * 20}x") for k in on), on
    _check_tower(_tower(600, 12, "fast", "fp16"), 4, 12, "C=600 fast")


# ------------------------------------------------------------------------------------------------ 3: arguments, fallbacks, state
def _launches(t, P, fn=None):
    eng, d = t.eng, t.dev
    eng.set_text_shared_prefix(P)
    eng.profile_begin(all_kernels=True)
    try:
        if fn is None:
            eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=True)
            eng.text_bwd(d["dfeat"])
        else:
            fn()
        torch.cuda.synchronize()
    finally:
        stats = eng.profile_end()
        eng.set_text_shared_prefix(0)
    return {k: v["launches"] for k, v in stats.items()}


def test_setter_refuses_bad_values_and_clamps_long_ones():
    lib = _lib()
    t = _tower(5, 20, "split_grad", "fp16")
    for bad in (-1, -7, t.L, t.L + 5):
        assert lib.lib.mvlpt_set_text_shared_prefix(t.eng.h, bad) == lib.ERR_ARG and "set_text_shared_prefix" in lib.last_error(t.eng.h), bad
    with pytest.raises(RuntimeError):
        t.eng.set_text_shared_prefix(-1)
    assert lib.lib.mvlpt_set_text_shared_prefix(None, 1) == lib.ERR_ARG
    # a prefix the gradient slots cannot hold is lowered, never refused: "end" shares 1 + 6 = 7 positions and Lg = max(eot) + 1 = 12
    # holds 6; what the engine ran shows in the row count of its GEMMs
    e = _Tower(5, 20, position="end", seed=43)
    assert e.P_layout == 7 and e.max_eot + 1 == 12
    f0, g0 = e.run(0)
    for grad_len, ran in ((12, 6), (20, 7)):
        f1, g1 = e.run(7, grad_len)
        assert torch.equal(f0, f1) and _rel(g1, g0) < DCTX_TOL, grad_len
        e.eng.set_text_grad_len(grad_len, e.max_eot)
        try:
            launches = _launches(e, 7)
        finally:
            e.eng.set_text_grad_len(e.L, 0)
        assert any(k.startswith(f"g{6 * (20 - ran)}x") for k in launches), (grad_len, ran, launches)


def test_default_is_off_and_zero_launches_what_an_untouched_engine_launches():
    fresh = _Tower(5, 20, seed=42)
    d, eng = fresh.dev, fresh.eng
    eng.profile_begin(all_kernels=True)
    eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=True)
    eng.text_bwd(d["dfeat"])
    torch.cuda.synchronize()
    untouched = {k: v["launches"] for k, v in eng.profile_end().items()}
    off, on = _launches(fresh, 0), _launches(fresh, fresh.P_layout)
    assert sum(untouched.values()) > 0 and untouched == off, (untouched, off)
    # with the prefix the GEMMs run over (C + 1) * (L - P) rows instead of C * L
    rows_off, rows_on = f"g{5 * 20}x", f"g{6 * (20 - fresh.P_layout)}x"
    assert any(k.startswith(rows_off) for k in off) and not any(k.startswith(rows_off) for k in on), on
    assert any(k.startswith(rows_on) for k in on), on


def test_every_fallback_route_ignores_the_setting():
    """ctx_per_class, deep prompts, the ranged entry, activation checkpointing: the launches and the bits of P = 0."""
    t = _tower(5, 20, "split_grad", "fp16")
    eng, d = t.eng, t.dev
    g = torch.Generator().manual_seed(5)
    ctx_csc = (torch.randn(t.C, N_CTX, 128, generator=g) * 0.1).to(DEV)
    ctx_deep = (torch.randn(1, N_CTX, 128, generator=g) * 0.1).to(DEV)
    ctx_grp = (torch.randn(2, N_CTX, 128, generator=g) * 0.1).to(DEV)
    dfeat_r = torch.randn(5, t.arch.embed_dim, generator=g).to(DEV)

    def csc():
        out["f"] = eng.text_fwd(d["prefix"], d["suffix"], ctx_csc, d["layout"], d["eot"], save_for_bwd=True).clone()
        out["g"] = eng.text_bwd(d["dfeat"]).clone()

    def deep():
        out["f"] = eng.text_fwd_deep(d["prefix"], d["suffix"], d["ctx"], ctx_deep, d["layout"], d["eot"], save_for_bwd=True).clone()
        out["g"] = torch.cat([x.reshape(-1) for x in eng.text_bwd_deep(d["dfeat"])]).clone()

    def ranged():
        out["f"] = eng.text_fwd_ranged(d["prefix"], d["suffix"], ctx_grp, d["layout"], d["eot"], [0, 2], [2, 5], save_for_bwd=True).clone()
        out["g"] = eng.text_bwd(dfeat_r).clone()

    def ckpt():
        eng.set_text_act_ckpt(2)
        try:
            out["f"] = eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=True).clone()
            out["g"] = eng.text_bwd(d["dfeat"]).clone()
        finally:
            eng.set_text_act_ckpt(1)

    ids = torch.randint(1, 1000, (t.C, t.L), generator=g, dtype=torch.int64)
    ids[:, 0], ids[torch.arange(t.C), t.eot.long()] = 49406, 49407        # SOS, and the EOT (the row maximum) where the prompts have it

    t.clip._ensure_token_embedding()      # (the token table is uploaded on first use: FrozenCLIP.encode_text does the same)

    def token_ids():
        out["f"] = eng.text_encode_tokens(ids).clone()
        out["g"] = out["f"]

    for fn in (csc, deep, ranged, ckpt, token_ids):
        res = []
        for P in (0, t.P_layout):
            out = {}
            res.append((_launches(t, P, fn), out["f"], out["g"]))
        assert res[0][0] == res[1][0], (fn.__name__, res[0][0], res[1][0])
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2]), fn.__name__


def test_sequences_longer_than_the_short_kernels_ignore_the_setting():
    """L = 84 > 80: the streamed attention kernels have no slot layout; the launches and the bits of P = 0."""
    t = _Tower(5, 84, seed=44)
    res = []
    for P in (0, t.P_layout):
        out = {}

        def step():
            out["f"], out["g"] = (x.clone() for x in (t.eng.text_fwd(t.dev["prefix"], t.dev["suffix"], t.dev["ctx"], t.dev["layout"],
                                                                         t.dev["eot"], save_for_bwd=True), t.eng.text_bwd(t.dev["dfeat"])))
        res.append((_launches(t, P, step), out["f"], out["g"]))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_the_setting_is_consumed_by_the_next_forward():
    """One-shot: the engine cannot check the claim against another call's tables, so a forward without a new call runs without a
    prefix, whichever entry consumed the setting."""
    t = _tower(5, 20, "split_grad", "fp16")
    eng, d = t.eng, t.dev
    rows_off, rows_on = f"g{5 * 20}x", f"g{6 * (20 - t.P_layout)}x"

    def fwd():
        eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=False)

    def two():
        fwd()
        fwd()
    first = _launches(t, t.P_layout, fwd)
    assert any(k.startswith(rows_on) for k in first) and not any(k.startswith(rows_off) for k in first), first
    both = _launches(t, t.P_layout, two)
    assert any(k.startswith(rows_on) for k in both) and any(k.startswith(rows_off) for k in both), both
    # a token-id forward consumes it too
    t.clip._ensure_token_embedding()
    eng.set_text_shared_prefix(t.P_layout)
    ids = torch.full((2, t.L), 5, dtype=torch.int64)
    ids[:, 0], ids[:, 7] = 49406, 49407
    eng.text_encode_tokens(ids)
    eng.profile_begin(all_kernels=True)
    fwd()
    torch.cuda.synchronize()
    after = {k: v["launches"] for k, v in eng.profile_end().items()}
    assert any(k.startswith(rows_off) for k in after) and not any(k.startswith(rows_on) for k in after), after


def test_a_forward_records_its_own_prefix():
    """A setting made after the forward does not reach that forward's backward, in either direction."""
    t = _tower(5, 20, "split_grad", "fp16")
    eng, d = t.eng, t.dev
    want = {P: t.run(P)[1] for P in (0, t.P_layout)}
    try:
        for at_fwd, at_bwd in ((t.P_layout, 0), (0, t.P_layout), (t.P_layout, 1)):
            eng.set_text_shared_prefix(at_fwd)
            eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=True)
            eng.set_text_shared_prefix(at_bwd)
            g = eng.text_bwd(d["dfeat"]).clone()
            assert torch.equal(g, want[at_fwd]), (at_fwd, at_bwd)
            assert torch.equal(eng.text_bwd(d["dfeat"]), want[at_fwd]), "a second backward on the same saved state"
    finally:
        eng.set_text_shared_prefix(0)


def test_a_forward_that_saves_nothing_shares_too():
    t = _tower(5, 20, "split_grad", "fp16")
    eng, d = t.eng, t.dev
    f0 = eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=False).clone()
    eng.set_text_shared_prefix(t.P_layout)
    try:
        f1 = eng.text_fwd(d["prefix"], d["suffix"], d["ctx"], d["layout"], d["eot"], save_for_bwd=False).clone()
    finally:
        eng.set_text_shared_prefix(0)
    torch.cuda.synchronize()
    assert torch.equal(f0, f1)


def test_models_set_the_prefix_of_their_class_table():
    """CustomCLIP tells the engine the prefix of its layout in front of the text forward; TEXT_SHARED_PREFIX = False tells it 0; the
    prompt gradient agrees inside the parity bound."""
    import tests.test_hip_model as M
    from mvlpt_amd.model import FrozenCLIP, shared_prefix_len
    from tests.golden_util import load_npz, t, tiny_state_dict
    case = load_npz("tiny_coop_cut")
    clip = FrozenCLIP(tiny_state_dict(), compute_dtype="fp16")
    seen, grads = [], {}
    setter = clip.engine.set_text_shared_prefix
    clip.engine.set_text_shared_prefix = lambda p: (seen.append(p), setter(p))[1]
    try:
        for on in (True, False):
            model = M.build_model(case, clip, 32, t(case["token_prefix"]), t(case["token_suffix"]))
            assert model.text_shared_prefix is True
            model.text_shared_prefix = on
            model.shared_prefix_min_rows = -10 ** 9   # (a handful of classes: under the default threshold the model would not share)
            pl = model.prompt_learner
            model.prompt_learner.zero_grad(set_to_none=True)
            logits = model(t(case["image"]).to(clip.device), task=None)
            model.cross_entropy(logits, t(case["label"]).to(clip.device)).backward()
            torch.cuda.synchronize()
            grads[on] = pl.ctx.grad.clone()
            want = shared_prefix_len(pl.layout, pl.token_prefix, pl.ctx.dim() == 2) if on else 0
            assert seen[-1] == want and (want > 0) == on, (seen, want)
    finally:
        setter(0)
    assert bool(grads[True].abs().max() > 0) and _rel(grads[True], grads[False]) < DCTX_TOL
