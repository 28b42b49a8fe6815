"""mvlpt_load_frozen / mvlpt_frozen_ready on the `tiny` architecture (-m gpu): the order in which a missing tensor is reported, loading
in any order, and every refusal with its text.  The order below is written out from the library's first_missing as it stood when the
loader and the readiness check still listed the names separately."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

ORDER = [
    "visual.conv1.weight",
    "visual.class_embedding",
    "visual.positional_embedding",
    "visual.ln_pre.weight",
    "visual.ln_pre.bias",
    "visual.ln_post.weight",
    "visual.ln_post.bias",
    "visual.proj",
    "positional_embedding",
    "ln_final.weight",
    "ln_final.bias",
    "text_projection",
    "visual.transformer.resblocks.0.attn.in_proj_weight",
    "visual.transformer.resblocks.0.attn.in_proj_bias",
    "visual.transformer.resblocks.0.attn.out_proj.weight",
    "visual.transformer.resblocks.0.attn.out_proj.bias",
    "visual.transformer.resblocks.0.mlp.c_fc.weight",
    "visual.transformer.resblocks.0.mlp.c_fc.bias",
    "visual.transformer.resblocks.0.mlp.c_proj.weight",
    "visual.transformer.resblocks.0.mlp.c_proj.bias",
    "visual.transformer.resblocks.0.ln_1.weight",
    "visual.transformer.resblocks.0.ln_1.bias",
    "visual.transformer.resblocks.0.ln_2.weight",
    "visual.transformer.resblocks.0.ln_2.bias",
    "visual.transformer.resblocks.1.attn.in_proj_weight",
    "visual.transformer.resblocks.1.attn.in_proj_bias",
    "visual.transformer.resblocks.1.attn.out_proj.weight",
    "visual.transformer.resblocks.1.attn.out_proj.bias",
    "visual.transformer.resblocks.1.mlp.c_fc.weight",
    "visual.transformer.resblocks.1.mlp.c_fc.bias",
    "visual.transformer.resblocks.1.mlp.c_proj.weight",
    "visual.transformer.resblocks.1.mlp.c_proj.bias",
    "visual.transformer.resblocks.1.ln_1.weight",
    "visual.transformer.resblocks.1.ln_1.bias",
    "visual.transformer.resblocks.1.ln_2.weight",
    "visual.transformer.resblocks.1.ln_2.bias",
    "visual.transformer.resblocks.2.attn.in_proj_weight",
    "visual.transformer.resblocks.2.attn.in_proj_bias",
    "visual.transformer.resblocks.2.attn.out_proj.weight",
    "visual.transformer.resblocks.2.attn.out_proj.bias",
    "visual.transformer.resblocks.2.mlp.c_fc.weight",
    "visual.transformer.resblocks.2.mlp.c_fc.bias",
    "visual.transformer.resblocks.2.mlp.c_proj.weight",
    "visual.transformer.resblocks.2.mlp.c_proj.bias",
    "visual.transformer.resblocks.2.ln_1.weight",
    "visual.transformer.resblocks.2.ln_1.bias",
    "visual.transformer.resblocks.2.ln_2.weight",
    "visual.transformer.resblocks.2.ln_2.bias",
    "transformer.resblocks.0.attn.in_proj_weight",
    "transformer.resblocks.0.attn.in_proj_bias",
    "transformer.resblocks.0.attn.out_proj.weight",
    "transformer.resblocks.0.attn.out_proj.bias",
    "transformer.resblocks.0.mlp.c_fc.weight",
    "transformer.resblocks.0.mlp.c_fc.bias",
    "transformer.resblocks.0.mlp.c_proj.weight",
    "transformer.resblocks.0.mlp.c_proj.bias",
    "transformer.resblocks.0.ln_1.weight",
    "transformer.resblocks.0.ln_1.bias",
    "transformer.resblocks.0.ln_2.weight",
    "transformer.resblocks.0.ln_2.bias",
    "transformer.resblocks.1.attn.in_proj_weight",
    "transformer.resblocks.1.attn.in_proj_bias",
    "transformer.resblocks.1.attn.out_proj.weight",
    "transformer.resblocks.1.attn.out_proj.bias",
    "transformer.resblocks.1.mlp.c_fc.weight",
    "transformer.resblocks.1.mlp.c_fc.bias",
    "transformer.resblocks.1.mlp.c_proj.weight",
    "transformer.resblocks.1.mlp.c_proj.bias",
    "transformer.resblocks.1.ln_1.weight",
    "transformer.resblocks.1.ln_1.bias",
    "transformer.resblocks.1.ln_2.weight",
    "transformer.resblocks.1.ln_2.bias",
]


@pytest.fixture(scope="module")
def tiny():
    from mvlpt_amd.weights import ARCHS, make_state_dict
    arch = ARCHS["tiny"]
    assert (arch.vision_layers, arch.transformer_layers) == (3, 2)
    return arch, make_state_dict(arch, seed=5, include_token_embedding=True)


def _load(eng, name, tensor):
    """One raw mvlpt_load_frozen call on the default stream; returns its code."""
    from mvlpt_amd import _lib
    tg = tensor.to(DEV).float().contiguous()
    shape = (C.c_int64 * max(tg.dim(), 1))(*tg.shape)
    rc = _lib.lib.mvlpt_load_frozen(eng.h, name.encode(), C.c_void_p(tg.data_ptr()), _lib.DT_F32, shape, tg.dim(), None)
    torch.cuda.synchronize()
    return rc


def _ready(eng):
    from mvlpt_amd import _lib
    rc = _lib.lib.mvlpt_frozen_ready(eng.h)
    return rc, (_lib.last_error(eng.h) if rc else "")


def _refusals(arch, sd):
    """(name, tensor, exact error text): every one is MVLPT_ERR_ARG."""
    d = arch.transformer_width
    return [
        ("visual.ln_pre.weight", torch.zeros(arch.vision_width + 1), "shape mismatch: visual.ln_pre.weight"),
        ("transformer.resblocks.1.mlp.c_fc.bias", torch.zeros(d), "shape mismatch for block tensor mlp.c_fc.bias"),
        ("transformer.resblocks.0.nope", torch.zeros(d), "unknown block tensor: nope"),
        ("visual.nope", torch.zeros(d), "unknown frozen tensor name: visual.nope"),
        ("transformer.resblocks.x.ln_1.weight", sd["transformer.resblocks.0.ln_1.weight"],
         "malformed block name: transformer.resblocks.x.ln_1.weight"),
        ("transformer.resblocks.9.ln_1.weight", sd["transformer.resblocks.0.ln_1.weight"], "layer index out of range"),
    ]


def _check_refusals(eng, arch, sd):
    from mvlpt_amd import _lib
    before = _ready(eng)
    for name, tensor, text in _refusals(arch, sd):
        assert _load(eng, name, tensor) == _lib.ERR_ARG, name
        assert _lib.last_error(eng.h) == text, name
        assert _ready(eng) == before, f"a refused load of {name} changed frozen_ready's answer"


def test_missing_tensors_are_reported_in_order(tiny):
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import Engine
    arch, sd = tiny
    assert sorted(ORDER) == sorted(k for k in sd if k not in ("logit_scale", "token_embedding.weight"))
    eng = Engine(arch, device=DEV)
    assert _ready(eng) == (_lib.ERR_STATE, "frozen tensor not loaded: " + ORDER[0])
    _check_refusals(eng, arch, sd)                       # on an empty handle
    for i, name in enumerate(ORDER):
        assert _load(eng, name, sd[name]) == 0, f"{name}: {_lib.last_error(eng.h)}"
        want = (_lib.ERR_STATE, "frozen tensor not loaded: " + ORDER[i + 1]) if i + 1 < len(ORDER) else (0, "")
        assert _ready(eng) == want, f"after {name}"
    _check_refusals(eng, arch, sd)                       # on a complete one
    eng.close()


def test_loading_in_reverse_order_gives_the_same_towers(tiny):
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import Engine
    arch, sd = tiny
    ref = Engine(arch, device=DEV)
    ref.load_frozen(sd)
    ref.load_token_embedding(sd["token_embedding.weight"])
    rev = Engine(arch, device=DEV)
    for name in reversed(list(sd)):                      # logit_scale (accepted, ignored) and the token table included
        assert _load(rev, name, sd[name]) == 0, f"{name}: {_lib.last_error(rev.h)}"
    assert _ready(rev) == (0, "")
    g = torch.Generator().manual_seed(11)
    image = torch.randn(2, 3, arch.image_resolution, arch.image_resolution, generator=g).to(DEV)
    ids = torch.randint(1, 1000, (3, arch.context_length), generator=g, dtype=torch.int32)
    for q, eot in enumerate((5, 76, 20)):
        ids[q, eot] = arch.vocab_size - 1
    img = [e.image_fwd(image).clone() for e in (ref, rev)]
    txt = [e.text_encode_tokens(ids).clone() for e in (ref, rev)]
    torch.cuda.synchronize()
    assert torch.equal(img[0], img[1]) and torch.equal(txt[0], txt[1])
    assert torch.isfinite(img[0]).all() and torch.isfinite(txt[0]).all()
    ref.close()
    rev.close()
