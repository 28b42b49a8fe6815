"""TEST-ONLY restatement of deep language prompting (TRAINER.MVLPT.COOP.N_DEEP, mvlpt_text_fwd / mvlpt_text_bwd with n_deep > 0) on the CPU.

It composes oracle.clip_oracle's own functions (assemble_prompts, block_fwd / block_bwd, layernorm_*, logits_*, cross_entropy_fwd_bwd,
the image encoder) with the two steps of the contract:

  forward   x_0 = assemble(ctx) + pos; in front of block l = 1 .. n_deep: x_l[c, ctx_pos[c, j], :] = ctx_deep[l - 1, j, :]
            (hidden states are REPLACED: no positional embedding; blocks behind n_deep run on whatever the previous block left)
  backward  with dx_l the gradient at the input of block l: dctx_deep[l - 1, j] = sum_c dx_l[c, ctx_pos[c, j]], and those rows of
            dx_l are then zero for the backward of block l - 1; dctx comes from dx_0 as ever.

The hand-written backward is checked against torch autograd in float64 by tests/test_deep_text_ref.py.  `forget_zeroing` and `add_pos`
build the two wrong variants that test tells apart.  The functions follow torch's default dtype (the oracle allocates with it)."""
from typing import Dict, Optional

import torch

from oracle import clip_oracle as O

# ---- the test architecture and inputs shared by tests/test_deep_text_ref.py and tests/test_hip_deep_text.py
TEXT_WIDTH, TEXT_HEADS, TEXT_LAYERS = 256, 4, 4
NAME_LENS = [1, 3, 2, 1, 4]          # C = 5 classes of unequal name lengths
N_CTX = 4
# Scale of the test's ctx_deep values, chosen on the CPU so that a no-op cannot hide: with rows of this size the restatement's text
# features with and without the deep prompts differ by 0.54 .. 0.66 of their largest entry and the logits of a whole step by
# 0.42 .. 0.68 (normalised as the bar), several hundred times the 1e-3 bar (tests/test_deep_text_ref.py and
# tests/test_hip_deep_text.py print and assert it).
CTX_DEEP_STD = 0.15


def deep_arch():
    """text width 256, 4 heads of 64, 4 text layers (a deep prompt meets a middle block, a checkpoint boundary and the compact last
    block); the `tiny` image tower"""
    from mvlpt_amd.weights import ARCHS, ClipArch
    t = ARCHS["tiny"]
    return ClipArch("deep_text_test", t.embed_dim, t.image_resolution, t.vision_layers, t.vision_width, t.vision_patch_size,
                    t.context_length, t.vocab_size, TEXT_WIDTH, TEXT_HEADS, TEXT_LAYERS)


def text_inputs(L: int, position: str, n_deep: int, seed: int = 5, n_ctx: int = N_CTX) -> Dict[str, torch.Tensor]:
    """prefix / suffix / ctx / ctx_deep / layout / eot / dfeat for C = len(NAME_LENS) sequences of L tokens (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    C_, dt = len(NAME_LENS), TEXT_WIDTH
    layout = O.build_prompt_layout(NAME_LENS, n_ctx, L, position)
    eot = torch.tensor([1 + n_ctx + k + 1 for k in NAME_LENS], dtype=torch.int64)      # SOT, ctx, name, '.', then EOT
    assert int(eot.max()) < L
    return {
        "prefix": torch.randn(C_, 1, dt, generator=g) * 0.02, "suffix": torch.randn(C_, L - 1 - n_ctx, dt, generator=g) * 0.02,
        "ctx": torch.randn(n_ctx, dt, generator=g) * 0.1,
        "ctx_deep": (torch.randn(n_deep, n_ctx, dt, generator=g) * CTX_DEEP_STD) if n_deep > 0 else None,
        "layout": layout, "eot": eot, "dfeat": torch.randn(C_, deep_arch().embed_dim, generator=g),
    }


def ctx_positions(layout: torch.Tensor, n_ctx: int) -> torch.Tensor:
    """ctx_pos[c, j] = the row of context token j in sequence c (what launch_build_ctx_pos builds from `layout`), int64 [C, n_ctx]."""
    C_, L = layout.shape
    pos = torch.full((C_, n_ctx), -1, dtype=torch.int64)
    for c in range(C_):
        for i in range(L):
            e = int(layout[c, i])
            if e < 0:
                pos[c, -e - 1] = i
    assert bool((pos >= 0).all())
    return pos


def _text_layers(sd) -> int:
    return len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks")})


def text_fwd_deep(sd, ctx, ctx_deep, prefix, suffix, layout, eot, *, heads: int, need_bwd: bool = True, add_pos: bool = False):
    """Features [C, e] and what text_bwd_deep needs.  ctx_deep [n_deep, n_ctx, dt] or None.  Differentiable torch ops throughout.
    add_pos (WRONG on purpose): adds the positional embedding to the replaced rows."""
    C_, L = layout.shape
    n_ctx = ctx.shape[0]
    n_deep = 0 if ctx_deep is None else ctx_deep.shape[0]
    layers = _text_layers(sd)
    assert n_deep <= layers - 1
    cp = ctx_positions(layout, n_ctx)
    rows_c = torch.arange(C_).unsqueeze(-1)
    x = O.assemble_prompts(ctx, prefix, suffix, layout) + sd["positional_embedding"][:L]
    saved = []
    for l in range(layers):
        if 1 <= l <= n_deep:
            new = ctx_deep[l - 1].expand(C_, -1, -1)
            if add_pos:
                new = new + sd["positional_embedding"][:L][cp]
            x = x.clone()
            x[rows_c, cp] = new
        x, s = O.block_fwd(x, sd, f"transformer.resblocks.{l}.", heads, causal=True)
        saved.append(s if need_bwd else None)
    rows = x[torch.arange(C_), eot]
    y, lnf = O.layernorm_fwd(rows, sd["ln_final.weight"], sd["ln_final.bias"])
    return y @ sd["text_projection"], (saved, lnf, eot, x.shape, cp, n_deep, layout, tuple(ctx.shape))


def text_bwd_deep(sd, dfeat, tctx, *, forget_zeroing: bool = False):
    """(dctx [n_ctx, dt], dctx_deep [n_deep, n_ctx, dt] or None).  forget_zeroing (WRONG on purpose): the overwritten rows keep
    carrying their gradient into the block in front."""
    saved, lnf, eot, xshape, cp, n_deep, layout, ctx_shape = tctx
    C_ = xshape[0]
    rows_c = torch.arange(C_).unsqueeze(-1)
    drows = O.layernorm_bwd(dfeat @ sd["text_projection"].t(), lnf[0], lnf[1], sd["ln_final.weight"])
    dx = torch.zeros(xshape)
    dx[torch.arange(C_), eot] = drows
    ddeep = torch.zeros(n_deep, ctx_shape[0], xshape[-1]) if n_deep > 0 else None
    for l in reversed(range(len(saved))):
        dx = O.block_bwd(dx, saved[l], sd, f"transformer.resblocks.{l}.")
        if 1 <= l <= n_deep:
            ddeep[l - 1] = dx[rows_c, cp].sum(0)
            if not forget_zeroing:
                dx = dx.clone()
                dx[rows_c, cp] = 0
    return O.scatter_prompt_grad(dx, layout, ctx_shape), ddeep


def step_deep(sd, *, image, label, vision_heads: int, text_heads: int, prefix, suffix, eot, layout, ctx, ctx_deep,
              vpt: Optional[torch.Tensor] = None, vpt_deep: Optional[torch.Tensor] = None, mask=None, need_grads: bool = True):
    """One CustomCLIP step with deep text prompts (and, optionally, visual prompts beside them under PROJECT_METHOD identity):
    {"img", "txt", "logits", "loss", "grads": {"ctx", "ctx_deep", ("vpt_embeddings", "vpt_embeddings_deep")}}."""
    with torch.no_grad():
        img, ictx = O.image_encoder_fwd(sd, image, vpt, vpt_deep, heads=vision_heads, need_bwd=need_grads and vpt is not None)
        txt, tctx = text_fwd_deep(sd, ctx, ctx_deep, prefix, suffix, layout, eot, heads=text_heads, need_bwd=need_grads)
        logits, lctx = O.logits_fwd(img, txt, float(sd["logit_scale"].exp()), mask)
        loss, dlogits = O.cross_entropy_fwd_bwd(logits, label)
        out = {"img": img, "txt": txt, "logits": logits, "loss": loss, "grads": {}}
        if not need_grads:
            return out
        dimg, dtxt = O.logits_bwd(dlogits, lctx)
        g_ctx, g_deep = text_bwd_deep(sd, dtxt, tctx)
        out["grads"]["ctx"] = g_ctx
        if g_deep is not None:
            out["grads"]["ctx_deep"] = g_deep
        if vpt is not None:
            g_vpt, g_vdeep = O.image_encoder_bwd(sd, dimg, ictx)
            out["grads"]["vpt_embeddings"] = g_vpt
            if g_vdeep is not None:
                out["grads"]["vpt_embeddings_deep"] = g_vdeep
    return out
