"""CPU checks of the host side of deep language prompting (TRAINER.MVLPT.COOP.N_DEEP): the configuration default, the prompt learner's
parameter and state-dict keys, same-seed equality of every existing parameter, the refusals at construction (raised before an engine
is touched), the flat optimizer buffers, and the autograd bridge + evaluation cache on a stub engine (the CPU oracle behind the
engine's method names, tests/fake_engine.py, with the two deep text methods added here from tests/deep_text_ref.py)."""
import pytest
import torch

from tests import deep_text_ref as R
from tests.fake_engine import OracleEngine, OracleFrozenCLIP

NAMES = ["dog", "great white shark", "grand piano", "cat", "big old oak tree"]


class DeepOracleEngine(OracleEngine):
    """OracleEngine + Engine.text_fwd_deep / text_bwd_deep; counts the text forwards it runs"""
    text_forwards = 0

    def text_fwd(self, *a, **k):
        self.text_forwards += 1
        return super().text_fwd(*a, **k)

    def text_fwd_deep(self, prefix, suffix, ctx, ctx_deep, layout, eot, save_for_bwd=False):
        self.text_forwards += 1
        with torch.no_grad():
            feat, self._dctx = R.text_fwd_deep(self.sd, ctx.detach(), None if ctx_deep is None else ctx_deep.detach(), prefix, suffix, layout,
                                               eot.long(), heads=self.arch.transformer_heads, need_bwd=save_for_bwd)
        return feat

    def text_bwd_deep(self, dfeat):
        with torch.no_grad():
            return R.text_bwd_deep(self.sd, dfeat, self._dctx)


class NoEngine:
    """Every refusal at construction must come before the engine is used: any attribute access fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the refusal")


def _clip(engine=None):
    from mvlpt_amd.weights import make_state_dict
    arch = R.deep_arch()
    sd = make_state_dict(arch, seed=11)
    clip = OracleFrozenCLIP(sd, arch)
    clip.engine = engine if engine is not None else DeepOracleEngine(sd, arch)
    return clip, sd, arch


def _cfg(n_deep=0, n_ctx=4, vpt=0, method="identity", csc=False, cocoop=0):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    T = cfg.TRAINER.MVLPT
    T.COOP.N_CTX, T.COOP.N_DEEP, T.COOP.CSC, T.COOP.CLASS_TOKEN_POSITION = n_ctx, n_deep, csc, "end"
    T.VPT.N_CTX, T.PROJECT_METHOD, T.PROJECT_DIM, T.COCOOP.N_CTX = vpt, method, 64, cocoop
    return cfg


def test_config_default_is_off():
    from mvlpt_amd.config import get_cfg_default
    assert get_cfg_default().TRAINER.MVLPT.COOP.N_DEEP == 0


def test_state_dict_keys_and_shape():
    from mvlpt_amd.model import MultitaskVLPromptLearner
    clip, _, arch = _clip()
    off = MultitaskVLPromptLearner(_cfg(0), NAMES, clip)
    on = MultitaskVLPromptLearner(_cfg(3), NAMES, clip)
    assert set(off.state_dict()) == {"ctx", "token_prefix", "token_suffix"}
    assert not hasattr(off, "ctx_deep") and off.coop_n_deep == 0
    assert set(on.state_dict()) == {"ctx", "ctx_deep", "token_prefix", "token_suffix"}
    assert tuple(on.ctx_deep.shape) == (3, 4, arch.transformer_width) and on.ctx_deep.dtype == torch.float32 and on.ctx_deep.requires_grad
    assert 0.015 < float(on.ctx_deep.detach().std()) < 0.025          # normal_(std=0.02)
    both = MultitaskVLPromptLearner(_cfg(2, vpt=2), NAMES, clip)
    assert set(both.state_dict()) == {"ctx", "ctx_deep", "vpt_embeddings", "vpt_embeddings_deep", "token_prefix", "token_suffix"}


@pytest.mark.parametrize("vpt", [0, 2])
def test_a_seed_gives_the_existing_parameters_the_same_values(vpt):
    """ctx_deep is drawn after every existing draw"""
    from mvlpt_amd.model import MultitaskVLPromptLearner
    clip, _, _ = _clip()
    torch.manual_seed(123)
    off = MultitaskVLPromptLearner(_cfg(0, vpt=vpt), NAMES, clip)
    torch.manual_seed(123)
    on = MultitaskVLPromptLearner(_cfg(2, vpt=vpt), NAMES, clip)
    a, b = dict(off.named_parameters()), dict(on.named_parameters())
    assert set(b) - set(a) == {"ctx_deep"}
    for k, v in a.items():
        assert torch.equal(v, b[k]), k


REFUSALS = [
    ("no context tokens", dict(n_deep=1, n_ctx=0), ValueError, "COOP.N_CTX is 0"),
    ("csc", dict(n_deep=1, csc=True), NotImplementedError, "COOP.CSC"),
    ("too deep", dict(n_deep=R.TEXT_LAYERS), ValueError, "transformer_layers - 1 = 3"),
    ("negative", dict(n_deep=-1), ValueError, "negative"),
    ("upt projection", dict(n_deep=1, vpt=2, method="transformer"), NotImplementedError, "UPT projection"),
    ("cocoop", dict(n_deep=1, n_ctx=0, cocoop=4), NotImplementedError, "COCOOP.N_CTX != 0"),
]


@pytest.mark.parametrize("kw,exc,text", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals_at_construction_name_their_cause(kw, exc, text):
    from mvlpt_amd import model as M
    from mvlpt_amd import mvlpt_cocoop as MC
    clip, _, _ = _clip(NoEngine())
    cfg = _cfg(**kw)
    classes = [M.MultitaskVLPromptLearner] + ([MC.MultitaskVLPromptLearner] if kw.get("cocoop") else [])
    for cls in classes:
        with pytest.raises(exc) as ei:
            cls(cfg, NAMES, clip)
        assert text in str(ei.value) and "N_DEEP" in str(ei.value)


def test_the_largest_depth_and_the_identity_projection_are_accepted():
    from mvlpt_amd.model import MultitaskVLPromptLearner
    clip, _, _ = _clip(NoEngine())
    pl = MultitaskVLPromptLearner(_cfg(R.TEXT_LAYERS - 1, vpt=2, method="identity"), NAMES, clip)
    assert pl.ctx_deep.shape[0] == R.TEXT_LAYERS - 1


def test_class_sharding_is_refused_with_deep_prompts():
    from mvlpt_amd.model import CustomCLIP
    clip, _, _ = _clip()
    model = CustomCLIP(_cfg(1), NAMES, clip)
    with pytest.raises(NotImplementedError, match="N_DEEP"):
        model.enable_class_sharding(0, 2)
    model.enable_class_sharding(0, 1)           # one rank: nothing is sharded
    CustomCLIP(_cfg(0), NAMES, clip).enable_class_sharding(0, 2)


def test_ctx_deep_is_in_the_flat_buffers_and_the_optimizer():
    from mvlpt_amd.distributed import FlatGradients, FlatParameters
    from mvlpt_amd.model import MultitaskVLPromptLearner
    from mvlpt_amd.trainer import build_optimizer
    clip, _, arch = _clip()
    pl = MultitaskVLPromptLearner(_cfg(2), NAMES, clip)
    n = sum(p.numel() for p in pl.parameters())
    assert n == 4 * arch.transformer_width * 3
    fp, fg = FlatParameters(pl.parameters()), FlatGradients(pl.parameters())
    flat_p = next(v for v in vars(fp).values() if torch.is_tensor(v) and v.numel() >= n)
    assert pl.ctx_deep.data_ptr() >= flat_p.data_ptr() and \
        pl.ctx_deep.data_ptr() + pl.ctx_deep.numel() * 4 <= flat_p.data_ptr() + flat_p.numel() * 4, "ctx_deep is not a view of the flat buffer"
    assert set(pl.state_dict()) == {"ctx", "ctx_deep", "token_prefix", "token_suffix"}
    cfg = _cfg(2)
    opt = build_optimizer(pl, cfg.OPTIM)
    assert any(p is pl.ctx_deep for grp in opt.param_groups for p in grp["params"])
    del fg


def _step(model, image, label):
    for p in model.parameters():
        p.grad = None
    logits = model(image)
    loss = model.cross_entropy(logits, label)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad.clone() for k, p in model.prompt_learner.named_parameters()}


@pytest.mark.parametrize("vpt", [0, 2])
def test_autograd_bridge_returns_the_gradient_of_ctx_deep(vpt):
    """CustomCLIP on the stub engine against the restatement's whole step: the bridge hands ctx_deep to the deep entries and its
    gradient back (the numbers are the oracle's on both sides: equality up to fp32 rounding)."""
    from mvlpt_amd.model import CustomCLIP
    clip, sd, arch = _clip()
    torch.manual_seed(2)
    model = CustomCLIP(_cfg(3, vpt=vpt), NAMES, clip)
    pl = model.prompt_learner
    assert pl.name_lens == R.NAME_LENS
    with torch.no_grad():
        pl.ctx_deep.mul_(R.CTX_DEEP_STD / 0.02)
    g = torch.Generator().manual_seed(9)
    image, label = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, len(NAMES), (4,), generator=g)
    logits, loss, grads = _step(model, image, label)
    P = {k: v.detach() for k, v in pl.named_parameters()}
    want = R.step_deep(sd, image=image, label=label, vision_heads=arch.vision_heads, text_heads=arch.transformer_heads,
                       prefix=pl.token_prefix, suffix=pl.token_suffix, eot=pl.eot.long(), layout=pl.layout, ctx=P["ctx"],
                       ctx_deep=P["ctx_deep"], vpt=P.get("vpt_embeddings"), vpt_deep=P.get("vpt_embeddings_deep"))
    assert set(grads) == set(want["grads"]) and "ctx_deep" in grads
    assert torch.allclose(logits, want["logits"], rtol=1e-5, atol=1e-5) and abs(float(loss) - float(want["loss"])) < 1e-5
    for k, gref in want["grads"].items():
        assert torch.allclose(grads[k].reshape(gref.shape), gref, rtol=1e-4, atol=1e-7 + 1e-5 * float(gref.abs().max())), k
    assert float(grads["ctx_deep"].abs().min(dim=-1).values.max()) > 0


def test_eval_cache_is_invalidated_by_a_change_of_ctx_deep_alone():
    from mvlpt_amd.model import CustomCLIP
    clip, _, _ = _clip()
    model = CustomCLIP(_cfg(2), NAMES, clip)
    eng = clip.engine
    model.prompt_learner.eval()
    image = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        a = model(image)
        assert eng.text_forwards == 1
        b = model(image)
        assert eng.text_forwards == 1 and torch.equal(a, b), "unchanged prompts: the cached text features are used"
        ctx_version = model.prompt_learner.ctx._version
        model.prompt_learner.ctx_deep.mul_(3.0)
        assert model.prompt_learner.ctx._version == ctx_version
        c = model(image)
    assert eng.text_forwards == 2, "a change of ctx_deep alone must run the text tower again"
    assert not torch.equal(a, c)


def test_ctx_deep_alone_can_carry_the_gradient():
    """A frozen ctx next to a trainable ctx_deep: the text tower still saves for a backward and ctx_deep gets its gradient."""
    from mvlpt_amd.model import CustomCLIP
    clip, _, _ = _clip()
    model = CustomCLIP(_cfg(2), NAMES, clip)
    model.prompt_learner.ctx.requires_grad_(False)
    g = torch.Generator().manual_seed(3)
    image, label = torch.randn(2, 3, 32, 32, generator=g), torch.randint(0, len(NAMES), (2,), generator=g)
    _, _, grads = _step_some(model, image, label)
    assert grads["ctx"] is None and grads["ctx_deep"] is not None and float(grads["ctx_deep"].abs().max()) > 0


def _step_some(model, image, label):
    for p in model.parameters():
        p.grad = None
    logits = model(image)
    loss = model.cross_entropy(logits, label)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in model.prompt_learner.named_parameters()}
