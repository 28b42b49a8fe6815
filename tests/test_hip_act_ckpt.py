"""Activation checkpointing of the text tower (-m gpu): TRAINER.ACT_CKPT / mvlpt_set_text_act_ckpt.

The recomputation inside text_bwd repeats the forward's launches, so wherever no LayerNorm is folded (towers under the row
threshold, text width < 256) a checkpointed step is held to the BITS of the un-checkpointed one, which in turn is held to the fp32
CPU oracle at the project's bar (max|d| <= 1e-3 max|ref|).  With folding active the two un-folded LayerNorms at a segment boundary
may move low bits, so each setting is held to the oracle on its own and to itself run to run.

Architectures are built by hand: the `tiny` one has two text layers, too few for a plan with several segments."""
import ctypes as C

import pytest
import torch

from tests.golden_util import load_npz, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-3
MODES = ["split_grad", "split_all", "fast"]          # split_grad is the engine's default


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _arch(text_width):
    from mvlpt_amd.weights import ClipArch
    # a two-block 128-wide image tower (never run here); 5 text layers: plans of 2, 3 and 5 segments differ
    return ClipArch(f"ckpt{text_width}", 128, 32, 2, 128, 16, 77, 49408, text_width, text_width // 64, 5)


class _Tower:
    """One engine, one set of plain-tower inputs, and the oracle's features / dctx for them (computed once, never changed)."""

    def __init__(self, text_width, C_, L, n, seed):
        from oracle import clip_oracle as O
        from mvlpt_amd.model import FrozenCLIP, build_prompt_layout
        from mvlpt_amd.weights import make_state_dict
        self.arch = _arch(text_width)
        self.sd = make_state_dict(self.arch, seed)
        self.clip = FrozenCLIP(self.sd, device=DEV)
        self.eng = self.clip.engine
        g = torch.Generator().manual_seed(seed)
        dt, e = text_width, self.arch.embed_dim
        name_lens = [1 + c % 3 for c in range(C_)]
        self.C, self.L, self.n = C_, L, n
        layout = build_prompt_layout(name_lens, n, L, "end")
        eot = torch.tensor([n + 3 + k for k in name_lens], dtype=torch.int32)
        prefix, suffix = torch.randn(C_, 1, dt, generator=g) * 0.02, torch.randn(C_, L - 1 - n, dt, generator=g) * 0.02
        ctx = torch.randn(n, dt, generator=g) * 0.1
        dfeat = torch.randn(C_, e, generator=g)
        with torch.no_grad():
            feat, tctx = O.text_encoder_fwd(self.sd, O.assemble_prompts(ctx, prefix, suffix, layout), eot.long(),
                                            heads=self.arch.transformer_heads)
            self.ref_feat = feat
            self.ref_dctx = O.scatter_prompt_grad(O.text_encoder_bwd(self.sd, dfeat, tctx), layout, tuple(ctx.shape))
        self.inputs = tuple(x.to(DEV) for x in (prefix, suffix, ctx, layout, eot))
        self.dfeat = dfeat.to(DEV)

    def step(self, n_seg):
        self.eng.set_text_act_ckpt(n_seg)
        try:
            f = self.eng.text_fwd(*self.inputs, save_for_bwd=True).clone()
            d = self.eng.text_bwd(self.dfeat).clone()
            torch.cuda.synchronize()
        finally:
            self.eng.set_text_act_ckpt(1)
        return f, d


@pytest.fixture(scope="module")
def small():
    return _Tower(128, 6, 20, 4, 21)          # 120 token rows: under fold_min_rows, and width < 256: nothing is folded


@pytest.fixture(scope="module")
def folded():
    return _Tower(256, 16, 77, 4, 22)         # 1 232 rows of width 256: LayerNorm folding is active


# ------------------------------------------------------------------------------------------------ 1: bit-equality
@pytest.mark.parametrize("mode", MODES)
def test_checkpointed_step_has_the_bits_of_the_saved_one(small, mode):
    small.eng.set_precision(mode)
    try:
        f1, d1 = small.step(1)
        ef, ed = _rel(f1, small.ref_feat), _rel(d1, small.ref_dctx)
        print(f"{mode}: n=1 against the oracle: features {ef:.2e}, dctx {ed:.2e}")
        assert ef <= TOL and ed <= TOL, f"{mode}: the un-checkpointed step is outside 1e-3 of the oracle: features {ef:.2e}, dctx {ed:.2e}"
        for n_seg in (2, 3, 5, 9):           # 9 clamps to the 5 layers
            f, d = small.step(n_seg)
            assert torch.equal(f, f1), f"{mode} n={n_seg}: features differ from n=1"
            assert torch.equal(d, d1), f"{mode} n={n_seg}: dctx differs from n=1"
    finally:
        small.eng.set_precision("split_grad")


# ------------------------------------------------------------------------------------------------ 2: folding active
def test_folded_tower_stays_within_the_oracle_bar_and_is_deterministic(folded):
    out = {}
    for n_seg in (1, 3):
        f, d = folded.step(n_seg)
        ef, ed = _rel(f, folded.ref_feat), _rel(d, folded.ref_dctx)
        print(f"folded n={n_seg} against the oracle: features {ef:.2e}, dctx {ed:.2e}")
        assert ef <= TOL and ed <= TOL, f"n={n_seg}: features {ef:.2e}, dctx {ed:.2e}"
        out[n_seg] = (f, d)
    f, d = folded.step(3)
    assert torch.equal(f, out[3][0]) and torch.equal(d, out[3][1]), "two checkpointed runs must be bit-identical"
    # the two settings differ by the two LayerNorms that are not folded at the segment boundaries (recorded in DESIGN.md; no bound)
    print(f"folded n=3 against n=1: features {_rel(out[3][0], out[1][0]):.2e}, dctx {_rel(out[3][1], out[1][1]):.2e}")


# ------------------------------------------------------------------------------------------------ 3: ranged, partial and full ranges
def _group_inputs(small, G):
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(23)
    C_, L, n, dt = 5, small.L, small.n, small.arch.transformer_width
    name_lens = [1, 2, 2, 1, 3]
    layout = build_prompt_layout(name_lens, n, L, "end").to(DEV)
    eot = torch.tensor([n + 3 + k for k in name_lens], dtype=torch.int32, device=DEV)
    prefix = (torch.randn(C_, 1, dt, generator=g) * 0.02).to(DEV)
    suffix = (torch.randn(C_, L - 1 - n, dt, generator=g) * 0.02).to(DEV)
    ctx = (torch.randn(G, n, dt, generator=g) * 0.1).to(DEV)
    return C_, g, (prefix, suffix, ctx, layout, eot)


def test_ranged_and_grouped_towers_keep_their_bits(small):
    """The ranged tower over partial ranges and over every range full (CoCoOp's per-image tower)."""
    eng, e = small.eng, small.arch.embed_dim
    lo, hi = [0, 2, 1], [2, 2, 5]                       # the second group is empty
    C_, g, inputs = _group_inputs(small, len(lo))
    S = sum(b - a for a, b in zip(lo, hi))
    dfeat_r, dfeat_g = torch.randn(S, e, generator=g).to(DEV), torch.randn(len(lo) * C_, e, generator=g).to(DEV)
    res = {}
    try:
        for n_seg in (1, 2):
            eng.set_text_act_ckpt(n_seg)
            fr = eng.text_fwd_ranged(*inputs, lo, hi, save_for_bwd=True).clone()
            dr = eng.text_bwd(dfeat_r).clone()
            fg = eng.text_fwd_ranged(*inputs, [0] * len(lo), [C_] * len(lo), save_for_bwd=True).clone()
            dg = eng.text_bwd(dfeat_g).clone()
            torch.cuda.synchronize()
            res[n_seg] = (fr, dr, fg, dg)
    finally:
        eng.set_text_act_ckpt(1)
    assert bool(res[1][1].abs().max() > 0) and torch.equal(res[1][1][1], torch.zeros_like(res[1][1][1])), "empty range: zero gradient"
    for a, b, what in zip(res[1], res[2], ("ranged features", "ranged dctx", "full-range features", "full-range dctx")):
        assert torch.equal(a, b), f"{what}: ACT_CKPT = 2 differs from ACT_CKPT = 1"


def _with_act_ckpt(make_cfg, n_seg):
    def cfg(*a, **k):
        c = make_cfg(*a, **k)
        c.TRAINER.ACT_CKPT = n_seg
        return c
    return cfg


def test_cocoop_step_keeps_its_bits_and_the_planner_sees_the_smaller_workspace(monkeypatch):
    import tests.test_cocoop_host as host
    from tests.test_hip_cocoop import build_cocoop, run_cocoop
    make_cfg, res = host.cocoop_cfg, {}
    try:
        for n_seg in (1, 2):
            monkeypatch.setattr(host, "cocoop_cfg", _with_act_ckpt(make_cfg, n_seg))
            model, image, label, _ = build_cocoop("tiny_cocoop")
            assert model.text_act_ckpt == n_seg and len(model.engine.text_act_ckpt_plan()) == n_seg
            res[n_seg] = run_cocoop(model, image, label)
            C_, L = model.prompt_learner.n_cls, model.prompt_learner.layout.shape[1]
            if n_seg == 1:
                budget = model.engine.text_workspace_bytes(4 * C_, L, True)
            model.max_text_workspace_bytes = budget            # what four images take when every layer is saved
            assert (model.images_per_chunk(8, L, True) == 4) if n_seg == 1 else (model.images_per_chunk(8, L, True) > 4)
    finally:
        model.engine.set_text_act_ckpt(1)
    (l1, s1, g1), (l2, s2, g2) = res[1], res[2]
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    assert set(g1) == set(g2) and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_mvlpt_cocoop_step_keeps_its_bits_and_the_planner_sees_the_smaller_workspace(monkeypatch):
    import tests.test_mvlpt_cocoop_host as host
    from tests.test_hip_mvlpt_cocoop import build_model, run_model
    make_cfg, res = host.mvlpt_cocoop_cfg, {}
    try:
        for n_seg in (1, 2):
            monkeypatch.setattr(host, "mvlpt_cocoop_cfg", _with_act_ckpt(make_cfg, n_seg))
            model, image, label, task, _ = build_model("tiny_mvlpt_cocoop_mask")
            assert model.text_act_ckpt == n_seg and len(model.engine.text_act_ckpt_plan()) == n_seg
            res[n_seg] = run_model(model, image, label, task)
            L = model.prompt_learner.layout.shape[1]
            if n_seg == 1:
                budget = model.engine.text_workspace_bytes(8, L, True)
            model.max_text_workspace_bytes = budget            # eight sequences when every layer is saved
            chunks = model.chunks([0] * 6, [2] * 6, L, True)   # six images of two sequences each
            assert (chunks[0][2] == 8) if n_seg == 1 else (chunks[0][2] > 8)
    finally:
        model.engine.set_text_act_ckpt(1)
    (l1, s1, g1), (l2, s2, g2) = res[1], res[2]
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    assert set(g1) == set(g2) and all(torch.equal(g1[k], g2[k]) for k in g1)


# ------------------------------------------------------------------------------------------------ 4: through the model
def test_model_on_the_reference_fixture(monkeypatch):
    """model.CustomCLIP on tiny_coop_cut (two text layers: one checkpointed, one saved): within the existing 1e-3 of the real
    reference's values, and the bits of ACT_CKPT = 1."""
    import tests.test_hip_model as M
    from mvlpt_amd.model import FrozenCLIP
    from tests.golden_util import tiny_state_dict
    case = load_npz("tiny_coop_cut")
    clip = FrozenCLIP(tiny_state_dict(), compute_dtype="fp16")
    make_cfg, res = M.cfg_for_case, {}
    for n_seg in (1, 2):
        monkeypatch.setattr(M, "cfg_for_case", _with_act_ckpt(make_cfg, n_seg))
        model = M.build_model(case, clip, 32, t(case["token_prefix"]), t(case["token_suffix"]))
        assert model.text_act_ckpt == n_seg and model.engine.text_act_ckpt_plan() == ([(0, 2, False)] if n_seg == 1 else [(0, 1, True), (1, 2, False)])
        err, worst = M.run_case(case, model, t(case["image"]), M.TOL_TINY_FP16, M.GRAD_TOL_FP16)        # logits, loss, gradients: 1e-3
        print(f"tiny_coop_cut ACT_CKPT={n_seg}: logits {err:.2e} grads {max(worst.values()):.2e}")
        dev = clip.device
        assert "task" not in case and t(case["label"]).dtype == torch.int64
        model.prompt_learner.zero_grad(set_to_none=True)
        logits = model(t(case["image"]).to(dev), task=None)
        loss = model.cross_entropy(logits, t(case["label"]).to(dev))
        loss.backward()
        torch.cuda.synchronize()
        res[n_seg] = (logits.detach().clone(), loss.detach().clone(), model.prompt_learner.ctx.grad.clone())
    for a, b, what in zip(res[1], res[2], ("logits", "loss", "grad_ctx")):
        assert torch.equal(a, b), f"{what}: ACT_CKPT = 2 differs from ACT_CKPT = 1"


# ------------------------------------------------------------------------------------------------ 5: workspace
def _align256(n):
    return (n + 255) & ~255


def _per_layer_and_boundary(arch, C_, L, X):
    """The six per-layer terms of the engine's carve_tower (x twice, qkv, attn, lse, u) and one fp32 boundary buffer."""
    T, d, H = C_ * L, arch.transformer_width, arch.transformer_heads
    x = _align256(T * d * 4)
    return 2 * x + _align256(T * 3 * d * 2 * X) + _align256(T * d * 2 * X) + _align256(C_ * H * L * 4) + _align256(T * 4 * d * 2), x


def _check_workspace_figures(eng, arch, C_, L):
    from mvlpt_amd.model import checkpoint_segments
    layers = arch.transformer_layers
    per_layer, boundary = _per_layer_and_boundary(arch, C_, L, 2)         # default mode: split operands (hi|lo pairs)
    try:
        eng.set_text_act_ckpt(1)
        b1 = eng.text_workspace_bytes(C_, L, True)
        nosave = eng.text_workspace_bytes(C_, L, False)
        for k in range(2, layers + 1):
            eng.set_text_act_ckpt(k)
            m_k = max(b - a for a, b, _ in checkpoint_segments(layers, k))
            bk = eng.text_workspace_bytes(C_, L, True)
            assert b1 - bk >= (layers - m_k) * per_layer - k * boundary, f"k={k}: {b1} -> {bk}"
            assert bk > nosave == eng.text_workspace_bytes(C_, L, False), "a forward that saves nothing is not affected"
    finally:
        eng.set_text_act_ckpt(1)
    assert eng.text_workspace_bytes(C_, L, True) == b1


def test_workspace_figures_small(small):
    _check_workspace_figures(small.eng, small.arch, small.C, small.L)


def test_workspace_figures_vit_b16_bytes_only():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    arch = ARCHS["ViT-B/16"]
    eng = Engine(arch, device=DEV)                       # no weights: nothing is launched
    _check_workspace_figures(eng, arch, 1000, 77)
    eng.close()


def test_a_checkpointed_forward_stays_inside_the_published_workspace(small):
    """The engine exposes no reservation query; its forward compares the carve with what it reserved (the published formula with
    the forward's own, smaller ctx table) and fails with MVLPT_ERR_STATE beyond it.  A fresh engine reserves exactly that figure, so
    a checkpointed step that runs on one, under every plan, stayed inside mvlpt_text_workspace_bytes."""
    from mvlpt_amd.model import FrozenCLIP
    f1, d1 = small.step(1)
    for n_seg in (5, 3, 2):
        eng = FrozenCLIP(small.sd, device=DEV).engine
        eng.set_text_act_ckpt(n_seg)
        f = eng.text_fwd(*small.inputs, save_for_bwd=True)
        d = eng.text_bwd(small.dfeat)
        torch.cuda.synchronize()
        assert torch.equal(f, f1) and torch.equal(d, d1), n_seg


# ------------------------------------------------------------------------------------------------ 6: state
def test_settings_plan_and_consumed_state(small):
    from mvlpt_amd import _lib
    from mvlpt_amd.model import checkpoint_segments
    eng = small.eng
    assert _lib.lib.mvlpt_set_text_act_ckpt(eng.h, 0) == _lib.ERR_ARG and "set_text_act_ckpt" in _lib.last_error(eng.h)
    with pytest.raises(RuntimeError):
        eng.set_text_act_ckpt(-2)
    assert eng.text_act_ckpt_plan() == [(0, 5, False)], "a refused setting changes nothing; the default is 1"
    try:
        for n_seg in range(1, 8):
            eng.set_text_act_ckpt(n_seg)
            assert eng.text_act_ckpt_plan() == checkpoint_segments(5, n_seg), n_seg
        first, n = (C.c_int32 * 2)(), C.c_int(0)
        eng.set_text_act_ckpt(3)
        assert _lib.lib.mvlpt_text_act_ckpt_plan(eng.h, first, 2, C.byref(n)) == _lib.ERR_ARG and n.value == 3
    finally:
        eng.set_text_act_ckpt(1)
    f1, d1 = small.step(1)

    # a forward keeps its own plan: changing the setting in front of the backward changes nothing
    for at_fwd, at_bwd in ((2, 1), (2, 5), (1, 3)):
        eng.set_text_act_ckpt(at_fwd)
        f = eng.text_fwd(*small.inputs, save_for_bwd=True).clone()
        eng.set_text_act_ckpt(at_bwd)
        d = eng.text_bwd(small.dfeat).clone()
        torch.cuda.synchronize()
        assert torch.equal(f, f1) and torch.equal(d, d1), (at_fwd, at_bwd)
        eng.set_text_act_ckpt(1)
        # the saved state: still there after an un-checkpointed backward, consumed by a checkpointed one
        dctx = torch.full_like(d1, 7.0)
        with torch.cuda.device(eng.device):
            rc = _lib.lib.mvlpt_text_bwd(eng.h, small.dfeat.data_ptr(), dctx.data_ptr(), None, None)
        torch.cuda.synchronize()
        if at_fwd == 1:
            assert rc == 0 and torch.equal(dctx, d1)
        else:
            assert rc == _lib.ERR_STATE and "consumed" in _lib.last_error(eng.h)
            assert bool((dctx == 7.0).all()), "a refused backward must not launch"
            with pytest.raises(RuntimeError, match="consumed"):
                eng.text_bwd(small.dfeat)
