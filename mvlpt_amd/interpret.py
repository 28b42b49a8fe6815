"""Prompt interpretation: the nearest vocabulary tokens of learned context vectors (scripts/interpret_prompt.py of the reference,
the analysis behind the nearest-words table of the CoOp paper).

The reference builds `torch.cdist(ctx, token_embedding)` [rows, 49408], argsorts all of it for the first `topk` columns and stops at
class-specific contexts (`raise NotImplementedError`, :61-63).  Here the distances and the selection are one HIP kernel against the
token table the engine already keeps (`Engine.nearest_tokens`, mvlpt_nearest_tokens): no [rows, vocab] matrix exists, so class-specific
contexts (n_cls * n_ctx rows) and CoCoOp's per-image contexts (B * n_ctx rows) cost what their rows cost.  Ties are decided: equal
distances order by token id (torch.argsort leaves them open).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from ._lib import NEAREST_MAX_K

CONTEXT_KEYS = ("ctx", "cocoop_ctx")                 # the context tensors of a prompt_learner state dict


def _check_topk(topk: int) -> int:
    topk = int(topk)
    if not 1 <= topk <= NEAREST_MAX_K:
        raise ValueError(f"topk must lie in [1, {NEAREST_MAX_K}] (MVLPT_NEAREST_MAX_K), got {topk}")
    return topk


def _nest(flat: list, shape: Sequence[int]):
    if len(shape) == 0:
        return flat[0]
    if len(shape) == 1:
        return flat
    step = len(flat) // shape[0] if shape[0] else 0
    return [_nest(flat[i * step:(i + 1) * step], shape[1:]) for i in range(shape[0])]


@torch.no_grad()
def nearest_words(clip, vectors: torch.Tensor, topk: int, tokenizer=None):
    """The `topk` nearest vocabulary words of every vector of `vectors` [..., text_width]: nested lists shaped like the leading
    dimensions, each leaf a list of (word, distance) by ascending (distance, token id).  `clip` is a FrozenCLIP (anything with an
    `engine.nearest_tokens` and, unless `tokenizer` is passed, a `tokenizer` with the `decoder` table the reference reads)."""
    topk = _check_topk(topk)
    tok = tokenizer if tokenizer is not None else clip.tokenizer
    v = torch.as_tensor(vectors).detach().float()
    if v.dim() == 0 or v.numel() == 0:
        raise ValueError(f"vectors must be [..., text_width] and not empty, got {tuple(v.shape)}")
    lead = tuple(v.shape[:-1])
    device = getattr(clip, "device", None)
    flat = v.reshape(-1, v.shape[-1])
    if device is not None:
        flat = flat.to(device)
    idx, dist = clip.engine.nearest_tokens(flat.contiguous(), topk)
    idx, dist = idx.cpu().tolist(), dist.cpu().tolist()
    decoder = tok.decoder
    rows = [[(decoder[i], float(x)) for i, x in zip(ri, rd)] for ri, rd in zip(idx, dist)]
    return _nest(rows, lead)


def interpret_state_dict(state_dict: Dict[str, torch.Tensor], clip, topk: int,
                         classnames: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """Nearest words of the context tensors of a `prompt_learner` checkpoint (its state dict, or the Dassl checkpoint dict around it):
      "ctx" [n_ctx, dt]          generic context       -> [words of vector 0, words of vector 1, ...]
      "ctx" [n_cls, n_ctx, dt]   class-specific (CSC)  -> {class label: [words of vector 0, ...]} (labels: `classnames`, or "class <c>")
      "cocoop_ctx" [n_ctx, dt]   the MVLPT CoCoOp route's static context, as the generic one.
    Every other key is ignored (`token_prefix` / `token_suffix` come from the class names, as the reference's load_model notes;
    `ctx_deep`, the deep text prompts, are hidden states of later blocks, not token embeddings, and have no nearest words)."""
    topk = _check_topk(topk)
    if isinstance(state_dict.get("state_dict"), dict):
        state_dict = state_dict["state_dict"]
    found = [k for k in CONTEXT_KEYS if isinstance(state_dict.get(k), torch.Tensor)]
    if not found:
        raise ValueError("no context tensor (" + " / ".join(CONTEXT_KEYS) + ") in the checkpoint; its keys: " + ", ".join(sorted(state_dict)))
    out: Dict[str, object] = {}
    for key in found:
        t = state_dict[key]
        if t.dim() == 2:
            out[key] = nearest_words(clip, t, topk)
        elif t.dim() == 3:
            if classnames is not None and len(classnames) != t.shape[0]:
                raise ValueError(f"{key} has {t.shape[0]} classes but {len(classnames)} class names were given")
            per_class = nearest_words(clip, t, topk)                             # one call: n_cls * n_ctx rows
            labels = list(classnames) if classnames is not None else [f"class {c}" for c in range(t.shape[0])]
            out[key] = dict(zip(labels, per_class))
        else:
            raise ValueError(f"{key} must be [n_ctx, width] or [n_cls, n_ctx, width], got {tuple(t.shape)}")
    return out


def format_lines(result) -> List[str]:
    """The reference's printed lines (scripts/interpret_prompt.py:56-59): `f"{m+1}: {words} {dist}"` with the words as a list of str
    and the distances as a list of `:.4f` strings.  `result` is what nearest_words returns for a [n, width] tensor; a dict (of
    interpret_state_dict, or its per-class dict) gives each entry's lines under a `name:` line, nested names joined by " / "."""
    if isinstance(result, dict):
        lines: List[str] = []
        for name, sub in result.items():
            if isinstance(sub, dict):
                for inner, rows in sub.items():
                    lines.append(f"{name} / {inner}:")
                    lines.extend(format_lines(rows))
            else:
                lines.append(f"{name}:")
                lines.extend(format_lines(sub))
        return lines
    lines = []
    for m, row in enumerate(result):
        words = [w for w, _ in row]
        dist = [f"{x:.4f}" for _, x in row]
        lines.append(f"{m+1}: {words} {dist}")
    return lines


@torch.no_grad()
def interpret_model(model, topk: int, classnames: Optional[Sequence[str]] = None) -> Dict[str, object]:
    """interpret_state_dict on a LIVE prompted model (mvlpt_amd.model / cocoop / mvlpt_cocoop CustomCLIP): its `ctx` / `cocoop_ctx`
    parameters as they are now, and under UPT also "ctx (projected)", the `coop_emb` of forward_mvlpt_proj — the contexts that actually
    enter the text tower, which the raw `ctx` only feeds."""
    import torch.nn as nn
    pl = model.prompt_learner
    sd = {k: getattr(pl, k).detach() for k in CONTEXT_KEYS if isinstance(getattr(pl, k, None), torch.Tensor)}
    out = interpret_state_dict(sd, model.clip_model, topk, classnames)
    proj = getattr(pl, "mvlpt_proj", None)
    if "ctx" in sd and proj is not None and not isinstance(proj, nn.Identity) and getattr(pl, "vpt_n_ctx", 0) != 0:
        coop_emb = pl.forward_mvlpt_proj(model.dtype)[0]
        out["ctx (projected)"] = interpret_state_dict({"ctx": coop_emb.detach()}, model.clip_model, topk, classnames)["ctx"]
    return out
