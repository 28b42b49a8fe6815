"""Deep language prompting on the HIP engine (-m gpu): mvlpt_text_fwd / mvlpt_text_bwd with n_deep > 0, Engine.text_fwd_deep / text_bwd_deep,
TRAINER.MVLPT.COOP.N_DEEP through CustomCLIP and the MVLPT trainer.

Expected values are computed at test time on the CPU by tests/deep_text_ref.py, which composes oracle.clip_oracle's own functions with
the overwrite and the gather-and-zero of the contract (include/mvlpt_hip.h) and is itself checked against float64 autograd by
tests/test_deep_text_ref.py.  The bar is the project's (tests/test_hip_model.py): max|a - b| <= 1e-3 max|ref| for features and every
gradient (logits: 1e-3 max(1, max|ref|), loss: 1e-3 absolute), fp16 towers in the default precision mode and in split_all; bf16 towers
are held to that file's bf16 bar (TOL_BF16 = 2.5e-2 / GRAD_TOL_BF16 = 6e-2: bf16 MFMA inputs round the frozen weights to 8 bits, on
every route of the project; measured here: features 3.8e-3 .. 5.4e-3, dctx 5.3e-3 .. 6.9e-3, dctx_deep 4.9e-3 .. 7.3e-3).

Architecture (built here, not in ARCHS): text width 256, 4 heads of 64, 4 text layers, so that a deep prompt meets a middle block, a
checkpoint boundary and the compact last block; the `tiny` image tower; C = 5 classes of unequal name lengths, n_ctx = 4; L = 77 and
the CUT_CONTEXTLEN length 11.  The test's ctx_deep rows have std R.CTX_DEEP_STD = 0.15, chosen on the CPU: the restatement's logits with
and without them differ by > 10 x the bar (test_deep_prompts_are_not_a_no_op asserts it on the figures it prints)."""
import ctypes as C

import pytest
import torch

from tests import deep_text_ref as R
from tests.test_hip_model import GRAD_TOL_BF16, TOL_BF16, TOL_FP16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = TOL_FP16            # 1e-3
CUT_L = 11
SEED = 11
NAMES = ["dog", "great white shark", "grand piano", "cat", "big old oak tree"]      # R.NAME_LENS words each


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _gelu_grad(u):
    return 0.5 * torch.erfc(-u * 0.7071067811865476) + u * (0.3989422804014327 * torch.exp(-0.5 * u * u))


class _Ref:
    """The restatement's features / dctx / dctx_deep per (L, position, n_deep, activation): computed once, never changed."""

    def __init__(self):
        from mvlpt_amd.weights import make_state_dict
        self.arch = R.deep_arch()
        self.sd = make_state_dict(self.arch, seed=SEED)
        self.cache = {}

    def get(self, L, position, n_deep, act="quick_gelu"):
        key = (L, position, n_deep, act)
        if key not in self.cache:
            from oracle import clip_oracle as O
            I = R.text_inputs(L, position, n_deep)
            mp = pytest.MonkeyPatch()
            try:
                if act == "gelu":      # the towers' activation replaced in the oracle, as tests/test_hip_gelu_towers.py does
                    mp.setattr(O, "quick_gelu", lambda u: torch.nn.functional.gelu(u))
                    mp.setattr(O, "quick_gelu_grad", _gelu_grad)
                with torch.no_grad():
                    feat, tctx = R.text_fwd_deep(self.sd, I["ctx"], I["ctx_deep"], I["prefix"], I["suffix"], I["layout"], I["eot"],
                                                 heads=R.TEXT_HEADS)
                    dctx, ddeep = R.text_bwd_deep(self.sd, I["dfeat"], tctx)
            finally:
                mp.undo()
            self.cache[key] = (I, feat, dctx, ddeep)
        return self.cache[key]


@pytest.fixture(scope="module")
def ref():
    return _Ref()


@pytest.fixture(scope="module")
def clips(ref):
    """one engine per (compute type, activation), made on first use"""
    from mvlpt_amd.model import FrozenCLIP, SyntheticTokenizer
    made = {}

    def get(dtype="fp16", act="quick_gelu"):
        if (dtype, act) not in made:
            made[(dtype, act)] = FrozenCLIP(ref.sd, compute_dtype=dtype, device=DEV, activation=act, tokenizer=SyntheticTokenizer())
        return made[(dtype, act)]
    return get


def _dev_inputs(I):
    return (I["prefix"].to(DEV), I["suffix"].to(DEV), I["ctx"].to(DEV), None if I["ctx_deep"] is None else I["ctx_deep"].to(DEV),
            I["layout"].to(DEV), I["eot"].to(torch.int32).to(DEV))


def _step(eng, I, save=True):
    feat = eng.text_fwd_deep(*_dev_inputs(I), save_for_bwd=save).clone()
    if not save:
        return feat, None, None
    dctx, ddeep = eng.text_bwd_deep(I["dfeat"].to(DEV))
    torch.cuda.synchronize()
    return feat, dctx.clone(), None if ddeep is None else ddeep.clone()


def _check(tag, got, want, tol=BAR, gtol=BAR):
    (f, d, dd), (_, rf, rd, rdd) = got, want
    e = {"features": rel(f, rf), "dctx": rel(d, rd), "dctx_deep": rel(dd, rdd)}
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["features"] <= tol, (tag, e)
    assert e["dctx"] <= gtol and e["dctx_deep"] <= gtol, (tag, e)
    return e


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("L", [77, CUT_L])
@pytest.mark.parametrize("position", ["end", "middle"])
@pytest.mark.parametrize("n_deep", [1, 2, 3])
def test_parity_with_the_restatement(ref, clips, n_deep, position, L):
    want = ref.get(L, position, n_deep)
    eng = clips().engine
    _check(f"n_deep {n_deep} {position} L {L}", _step(eng, want[0]), want)


# ------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("mode", ["split_grad", "split_all"])
def test_precision_modes(ref, clips, mode):
    eng = clips().engine
    eng.set_precision(mode)
    try:
        for n_deep, position in ((2, "middle"), (3, "end")):
            want = ref.get(77, position, n_deep)
            _check(f"{mode} n_deep {n_deep} {position}", _step(eng, want[0]), want)
    finally:
        eng.set_precision("split_grad")


def test_bf16_towers(ref, clips):
    """bf16 MFMA inputs round the frozen weights to 8 bits: the project's bf16 bar (tests/test_hip_model.py)"""
    eng = clips("bf16").engine
    for n_deep, position in ((1, "end"), (3, "middle")):
        want = ref.get(77, position, n_deep)
        _check(f"bf16 n_deep {n_deep} {position}", _step(eng, want[0]), want, TOL_BF16, GRAD_TOL_BF16)


def test_exact_gelu_towers(ref, clips):
    eng = clips("fp16", "gelu").engine
    for n_deep, position, L in ((2, "end", 77), (3, "middle", CUT_L)):
        want = ref.get(L, position, n_deep, "gelu")
        _check(f"gelu n_deep {n_deep} {position} L {L}", _step(eng, want[0]), want)
    # forced folding under the exact GELU (ln_1 folds, ln_2 stays a pass): the un-folded ln_1 behind an overwrite
    eng.set_ln_fold(2, 1)
    try:
        want = ref.get(77, "end", 2, "gelu")
        _check("gelu folded n_deep 2", _step(eng, want[0]), want)
    finally:
        eng.set_ln_fold(2, 1024)


@pytest.mark.parametrize("fold", ["off", "forced"])
@pytest.mark.parametrize("segments", [1, 2, 4])
def test_activation_checkpointing_and_layernorm_folding(ref, clips, segments, fold):
    """4 layers: 2 segments cut in front of block 2, 4 segments in front of every block, the last segment being the compact last block
    alone.  Without folding (385 and 55 token rows are under the row threshold) the recomputation repeats the forward's launches, so
    a checkpointed step has the bits of the saved one.  Forced folding: ln_1 of every block behind an overwrite stays un-folded, the
    later ones (n_deep 1: blocks 2 and 3) fold; each setting is held to the restatement."""
    eng = clips().engine
    if fold == "forced":
        eng.set_ln_fold(2, 1)
    try:
        for n_deep, position, L in ((3, "end", 77), (1, "middle", 77), (2, "end", CUT_L)):
            want = ref.get(L, position, n_deep)
            eng.set_text_act_ckpt(1)
            base = _step(eng, want[0])
            eng.set_text_act_ckpt(segments)
            got = _step(eng, want[0])
            _check(f"ckpt {segments} fold {fold} n_deep {n_deep} {position} L {L}", got, want)
            again = _step(eng, want[0])
            assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs of one setting are not bit-identical"
            if fold == "off":
                assert all(torch.equal(a, b) for a, b in zip(got, base)), f"ckpt {segments}: not the bits of the saved step"
    finally:
        eng.set_text_act_ckpt(1)
        eng.set_ln_fold(2, 1024)


@pytest.mark.parametrize("fold", ["off", "forced"])
def test_save_and_no_save_forwards_give_equal_features(ref, clips, fold):
    eng = clips().engine
    if fold == "forced":
        eng.set_ln_fold(2, 1)
    try:
        for n_deep, position in ((1, "end"), (3, "middle")):
            I = ref.get(77, position, n_deep)[0]
            a, _, _ = _step(eng, I, save=False)
            b, _, _ = _step(eng, I, save=True)
            assert torch.equal(a, b), f"fold {fold} n_deep {n_deep}: {rel(a, b):.2e}"
    finally:
        eng.set_ln_fold(2, 1024)


# ------------------------------------------------------------------------------------------------ no deep prompts: the plain entries' bits
@pytest.mark.parametrize("segments", [1, 2])
def test_no_deep_prompts_has_the_bits_of_the_plain_entries(ref, clips, segments):
    from mvlpt_amd import _lib
    eng = clips().engine
    I = ref.get(77, "middle", 0)[0]
    prefix, suffix, ctx, _, layout, eot = _dev_inputs(I)
    dfeat = I["dfeat"].to(DEV)
    eng.set_text_act_ckpt(segments)
    try:
        f0 = eng.text_fwd(prefix, suffix, ctx, layout, eot, save_for_bwd=True).clone()
        d0 = eng.text_bwd(dfeat).clone()
        f1 = eng.text_fwd_deep(prefix, suffix, ctx, None, layout, eot, save_for_bwd=True).clone()
        d1, dd1 = eng.text_bwd_deep(dfeat)
        assert dd1 is None and torch.equal(f0, f1) and torch.equal(d0, d1)
        # n_deep = 0 with a non-null ctx_deep pointer, straight through the C entries; the plain backward then accepts the state
        junk = torch.full((1, R.N_CTX, R.TEXT_WIDTH), float("nan"), device=DEV)
        f2, d2 = torch.empty_like(f0), torch.empty_like(d0)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: C.c_void_p(t.data_ptr())
        job = _lib.MvlptTextJob(prefix=prefix.data_ptr(), suffix=suffix.data_ptr(), ctx=ctx.data_ptr(), n_ctx=R.N_CTX, ctx_deep=junk.data_ptr(),
                                n_deep=0, layout=layout.data_ptr(), eot=eot.data_ptr(), n_cls=len(R.NAME_LENS), L=77, save_for_bwd=1)
        rc = _lib.lib.mvlpt_text_fwd(eng.h, C.byref(job), P(f2), st)
        assert rc == 0, _lib.last_error(eng.h)
        assert _lib.lib.mvlpt_text_bwd(eng.h, P(dfeat), P(d2), None, st) == 0, _lib.last_error(eng.h)
        torch.cuda.synchronize()
        assert torch.equal(f0, f2) and torch.equal(d0, d2)
    finally:
        eng.set_text_act_ckpt(1)


# ------------------------------------------------------------------------------------------------ the model: logits, loss, gradients
def _model(clips, n_deep, position, L_cut=False, vpt=0, dtype="fp16"):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import CustomCLIP
    clip = clips(dtype)
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (clip.arch.image_resolution,) * 2
    T = cfg.TRAINER.MVLPT
    T.COOP.N_CTX, T.COOP.N_DEEP, T.COOP.CLASS_TOKEN_POSITION = R.N_CTX, n_deep, position
    T.VPT.N_CTX, T.VPT.DEEP, T.PROJECT_METHOD = vpt, True, "identity"
    cfg.TRAINER.CUT_CONTEXTLEN = L_cut
    torch.manual_seed(3)
    model = CustomCLIP(cfg, NAMES, clip).to(DEV)
    pl = model.prompt_learner
    assert pl.name_lens == R.NAME_LENS and pl.layout.shape[1] == (CUT_L if L_cut else 77)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        pl.ctx.copy_(torch.randn(pl.ctx.shape, generator=g) * 0.1)
        if n_deep:
            pl.ctx_deep.copy_(torch.randn(pl.ctx_deep.shape, generator=g) * R.CTX_DEEP_STD)
    return model


def _model_ref(ref, model, image, label, with_deep=True, need_grads=True):
    pl = model.prompt_learner
    P = {k: v.detach().cpu() for k, v in pl.named_parameters()}
    return R.step_deep(ref.sd, image=image, label=label, vision_heads=ref.arch.vision_heads, text_heads=R.TEXT_HEADS,
                       prefix=pl.token_prefix.cpu(), suffix=pl.token_suffix.cpu(), eot=pl.eot.cpu().long(), layout=pl.layout.cpu(),
                       ctx=P["ctx"], ctx_deep=P.get("ctx_deep") if with_deep else None, vpt=P.get("vpt_embeddings"),
                       vpt_deep=P.get("vpt_embeddings_deep"), need_grads=need_grads)


def _batch(arch, B=6, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, arch.image_resolution, arch.image_resolution, generator=g), torch.randint(0, len(NAMES), (B,), generator=g)


def _check_step(tag, logits, loss, grads, want, tol=BAR, gtol=BAR):
    e = {"logits": float((logits.detach().cpu() - want["logits"]).abs().max()) / max(1.0, float(want["logits"].abs().max())),
         "loss": abs(float(loss.detach()) - float(want["loss"]))}
    assert set(grads) == set(want["grads"]), (sorted(grads), sorted(want["grads"]))
    for k, g in want["grads"].items():
        assert grads[k] is not None, f"no gradient for {k}"
        e["grad_" + k] = rel(grads[k].reshape(g.shape), g)
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["logits"] <= tol and e["loss"] <= tol, (tag, e)
    bad = {k: v for k, v in e.items() if k.startswith("grad_") and v > gtol}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("n_deep,position,cut", [(1, "end", False), (2, "middle", True), (3, "middle", False), (3, "end", True)])
def test_model_logits_loss_and_gradients(ref, clips, n_deep, position, cut):
    model = _model(clips, n_deep, position, cut)
    image, label = _batch(ref.arch)
    logits = model(image.to(DEV))
    loss = model.cross_entropy(logits, label.to(DEV))
    loss.backward()
    want = _model_ref(ref, model, image, label)
    assert set(want["grads"]) == {"ctx", "ctx_deep"}
    _check_step(f"model n_deep {n_deep} {position} cut {cut}", logits, loss,
                {k: p.grad for k, p in model.prompt_learner.named_parameters()}, want)


def test_deep_prompts_are_not_a_no_op(ref, clips):
    """By the restatement's own figures the logits with and without the deep prompts differ by more than 10 x the bar, so an engine
    that ignored ctx_deep could not pass the parity tests; the engine's logits are on the right side of that gap."""
    for n_deep in (1, 2, 3):
        model = _model(clips, n_deep, "end")
        image, label = _batch(ref.arch)
        a = _model_ref(ref, model, image, label, need_grads=False)["logits"]
        b = _model_ref(ref, model, image, label, with_deep=False, need_grads=False)["logits"]
        gap = float((a - b).abs().max()) / max(1.0, float(a.abs().max()))
        print(f"n_deep {n_deep}: restatement logits with / without deep prompts differ by {gap:.3e} (normalised as the bar)")
        assert gap > 10 * BAR
        with torch.no_grad():
            got = model(image.to(DEV)).cpu()
        assert float((got - a).abs().max()) / max(1.0, float(a.abs().max())) <= BAR


def test_eval_text_cache_follows_ctx_deep(ref, clips):
    model = _model(clips, 2, "end")
    model.prompt_learner.eval()
    image, _ = _batch(ref.arch)
    with torch.no_grad():
        a = model(image.to(DEV)).clone()
        ver = model.text_cache.eval_key
        b = model(image.to(DEV)).clone()
        assert model.text_cache.eval_key == ver and torch.equal(a, b)
        model.prompt_learner.ctx_deep.mul_(0.5)
        c = model(image.to(DEV))
    assert model.text_cache.eval_key != ver and not torch.equal(a, c)


def test_class_sharding_is_refused(clips):
    model = _model(clips, 1, "end")
    with pytest.raises(NotImplementedError, match="N_DEEP"):
        model.enable_class_sharding(0, 2)


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(tmp_path, ref, vpt):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"          # the name is not read: the architecture comes from the state dict handed over below
    cfg.INPUT.SIZE = (32, 32)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 6
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.LR, cfg.OPTIM.WARMUP_EPOCH, cfg.TRAIN.PRINT_FREQ = 1, 0.05, 0, 1000
    T = cfg.TRAINER.MVLPT
    T.COOP.N_CTX, T.COOP.N_DEEP, T.COOP.CLASS_TOKEN_POSITION = R.N_CTX, 3, "end"
    if vpt:
        T.VPT.N_CTX, T.VPT.DEEP, T.PROJECT_METHOD = 2, True, "identity"
    dm = SyntheticDataManager(cfg, len(NAMES), 2, device="cuda", seed=3)
    torch.manual_seed(5)
    return MVLPT(cfg, dm=dm, clip_state_dict=ref.sd)


@pytest.mark.parametrize("vpt", [False, True], ids=["text_only", "independent_vl"])
def test_trainer_step(tmp_path, ref, vpt):
    """One MVLPT step with COOP.N_DEEP 3 alone, and next to VPT.DEEP under PROJECT_METHOD identity (independent V-L prompting):
    loss and every gradient within the bar of the restatement on the parameters before the step; the optimizer moves ctx_deep."""
    tr = _trainer(tmp_path, ref, vpt)
    pl = tr.model.prompt_learner
    names = {k for k, _ in pl.named_parameters()}
    assert names == ({"ctx", "ctx_deep", "vpt_embeddings", "vpt_embeddings_deep"} if vpt else {"ctx", "ctx_deep"})
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        pl.ctx_deep.copy_(torch.randn(pl.ctx_deep.shape, generator=g) * R.CTX_DEEP_STD)
    batch = tr.train_loader_x[0] if hasattr(tr.train_loader_x, "__getitem__") else next(iter(tr.train_loader_x))
    image, label = batch["img"].cpu(), batch["label"].cpu()
    want = _model_ref(ref, tr.model, image, label)
    before = {k: p.detach().clone() for k, p in pl.named_parameters()}
    tr.set_model_mode("train")
    tr.epoch, tr.num_batches, tr.batch_idx = 0, 10, 0
    out = tr.forward_backward(batch)
    torch.cuda.synchronize()
    e = abs(float(out["loss"]) - float(want["loss"]))
    print(f"trainer vpt={vpt}: loss err {e:.2e}")
    assert e <= BAR
    for k, gref in want["grads"].items():
        got = dict(pl.named_parameters())[k].grad
        assert got is not None, k
        err = rel(got.reshape(gref.shape), gref)
        print(f"   grad {k}: {err:.2e}")
        assert err <= BAR, (k, err)
    moved = float((pl.ctx_deep.detach() - before["ctx_deep"]).abs().max())
    assert moved > 0.0, "the optimizer did not move ctx_deep"
    assert set(pl.state_dict()) >= {"ctx", "ctx_deep", "token_prefix", "token_suffix"}


# ------------------------------------------------------------------------------------------------ C-level refusals
def test_c_level_refusals_leave_the_outputs_alone(ref, clips):
    from mvlpt_amd import _lib
    eng = clips().engine
    I = ref.get(77, "end", 2)[0]
    prefix, suffix, ctx, deep, layout, eot = _dev_inputs(I)
    dfeat = I["dfeat"].to(DEV)
    Cn, e = len(R.NAME_LENS), ref.arch.embed_dim
    SENT = 777.0
    feat = torch.full((Cn, e), SENT, device=DEV)
    dctx = torch.full((R.N_CTX, R.TEXT_WIDTH), SENT, device=DEV)
    ddeep = torch.full((2, R.N_CTX, R.TEXT_WIDTH), SENT, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lib = _lib.lib

    def fwd(ctx_, n_ctx, deep_, n_deep, suffix_=suffix, layout_=layout, save=1):
        D = lambda t: None if t is None else t.data_ptr()
        job = _lib.MvlptTextJob(prefix=D(prefix), suffix=D(suffix_), ctx=D(ctx_), n_ctx=n_ctx, ctx_deep=D(deep_), n_deep=n_deep,
                                layout=D(layout_), eot=D(eot), n_cls=Cn, L=77, save_for_bwd=save)
        return lib.mvlpt_text_fwd(eng.h, C.byref(job), P(feat), st)

    too_deep = torch.zeros(R.TEXT_LAYERS, R.N_CTX, R.TEXT_WIDTH, device=DEV)
    assert fwd(ctx, R.N_CTX, too_deep, R.TEXT_LAYERS) == _lib.ERR_ARG and "text_layers - 1" in _lib.last_error(eng.h)
    assert fwd(ctx, R.N_CTX, None, 2) == _lib.ERR_ARG and "ctx_deep is null" in _lib.last_error(eng.h)
    I0 = R.text_inputs(77, "end", 0, n_ctx=0)
    assert fwd(None, 0, deep, 2, I0["suffix"].to(DEV), I0["layout"].to(DEV)) == _lib.ERR_ARG and "n_ctx == 0" in _lib.last_error(eng.h)
    assert fwd(ctx, R.N_CTX, deep, -1) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((feat == SENT).all()), "a refused forward wrote its output"

    # the backward without dctx_deep after a deep forward (the plain and the deep backward are one entry): refused; nothing is written
    assert fwd(ctx, R.N_CTX, deep, 2) == 0, _lib.last_error(eng.h)
    assert lib.mvlpt_text_bwd(eng.h, P(dfeat), P(dctx), None, st) == _lib.ERR_ARG and "dctx_deep is null" in _lib.last_error(eng.h)
    torch.cuda.synchronize()
    assert bool((dctx == SENT).all()) and bool((ddeep == SENT).all()), "a refused backward wrote its outputs"
    # ... and the state is still good for the right call
    assert lib.mvlpt_text_bwd(eng.h, P(dfeat), P(dctx), P(ddeep), st) == 0, _lib.last_error(eng.h)
    torch.cuda.synchronize()
    want = ref.get(77, "end", 2)
    assert rel(dctx, want[2]) <= BAR and rel(ddeep, want[3]) <= BAR

    # the backward after a plain forward takes a null dctx_deep
    plain = eng.text_fwd(prefix, suffix, ctx, layout, eot, save_for_bwd=True)
    assert lib.mvlpt_text_bwd(eng.h, P(dfeat), P(dctx), None, st) == 0, _lib.last_error(eng.h)
    torch.cuda.synchronize()
    assert torch.equal(dctx, eng.text_bwd(dfeat))
    del plain

