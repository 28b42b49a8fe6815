"""Host-side mirror of the reference's prompted-CLIP model API (trainers/mvlpt.py:138-583), MI355X-native.

Same class names, constructor arguments, attribute names and — most importantly — the same
``prompt_learner.state_dict()`` keys (``ctx``, ``vpt_embeddings``, ``vpt_embeddings_deep``, ``token_prefix``,
``token_suffix``, ``mvlpt_proj.resblocks.0.*``, ``mvlpt_proj_ctx_{coop,vpt}_{pre,post}.*``), so checkpoints
interoperate and ``self.model(image, task=…)`` / ``self.model.prompt_learner`` work under the trainer exactly
as in the reference.  The towers do NOT run on PyTorch ops: `CustomCLIP.forward` is one
``torch.autograd.Function`` whose forward/backward call libmvlpt_hip.so (hand-written gfx950 kernels).  Only the
tiny UPT projection (forward_mvlpt_proj, ≤52 tokens × width 128, trainable weights) stays on torch autograd.

Deviations (documented in DESIGN.md): prompt parameters are kept in fp32 even when PREC == "fp16" (fp32 master
copies; the reference keeps fp16 parameters and has no loss scaling).  CoCoOp inside MVLPT (MVLPT.COCOOP.N_CTX != 0) is not this
module's route: it lives in mvlpt_amd/mvlpt_cocoop.py, and trainers/cocoop.py's own CoCoOp in mvlpt_amd/cocoop.py.
"""
from __future__ import annotations

import math
import os
import weakref
from collections import OrderedDict
from functools import reduce
from operator import mul
from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from ._lib import TEXT_MIN_L
from .engine import Engine
from .schedule import ImagePrefetch, TextFeatureCache, check_forward_is_current, fork
from .weights import ClipArch, _randn, arch_from_state_dict, is_resnet

# compute units of the text tower's partition in the two-tower pipeline (CustomCLIP.set_cu_partition); 0 = no partition.
# Overridden by the environment variable MVLPT_TEXT_CUS.
DEFAULT_TEXT_CUS = 0

SOT_TOKEN, EOT_TOKEN = 49406, 49407     # clip/simple_tokenizer.py: <|startoftext|>, <|endoftext|>
X_TOKEN = 343                            # "X" placeholder word (trainers/mvlpt.py:227), from tests/golden/tokens.npz


# ------------------------------------------------------------------------------------------------ tokenisation
_DEFAULT_TOKENIZER = None


def default_tokenizer():
    """The real thing: own byte-level BPE over the shipped merge table (mvlpt_amd/tokenizer.py), ids bit-exact against the
    reference tokenizer (tests/test_tokenizer.py)."""
    global _DEFAULT_TOKENIZER
    if _DEFAULT_TOKENIZER is None:
        from .tokenizer import BPETokenizer
        _DEFAULT_TOKENIZER = BPETokenizer()
    return _DEFAULT_TOKENIZER


class SyntheticTokenizer:
    """Hash-based stand-in for clip.simple_tokenizer, kept for tests that want token ids independent of any table (rounds 1-2
    used it wherever the BPE merge table was missing; the table ships now and `FrozenCLIP` defaults to the real tokenizer).
    One pseudo-token per whitespace-separated word (stable hash), which reproduces the
    *structure* the hot path depends on: [SOT, prefix words…, name words…, '.', EOT, 0…] and name_lens."""

    def encode(self, text: str) -> List[int]:
        out = []
        for w in text.replace(".", " .").split():
            if w == "X":
                out.append(X_TOKEN)
            elif w == ".":
                out.append(269)
            else:
                h = 0
                for ch in w.lower():
                    h = (h * 131 + ord(ch)) % 40000
                out.append(1000 + h)
        return out

    def tokenize(self, texts, context_length: int = 77) -> torch.Tensor:
        """Same contract as clip.tokenize (clip/clip.py:187-223)."""
        if isinstance(texts, str):
            texts = [texts]
        res = torch.zeros(len(texts), context_length, dtype=torch.long)
        for i, t in enumerate(texts):
            ids = [SOT_TOKEN] + self.encode(t) + [EOT_TOKEN]
            if len(ids) > context_length:
                raise RuntimeError(f"Input {t} is too long for context length {context_length}")
            res[i, :len(ids)] = torch.tensor(ids)
        return res


class PretokenizedPrompts:
    """Token ids produced elsewhere (e.g. by the reference tokenizer, stored in a fixture)."""

    def __init__(self, tokenized_prompts: torch.Tensor, name_lens: Sequence[int]):
        self.tokenized_prompts = tokenized_prompts.long()
        self.name_lens = [int(x) for x in name_lens]


def build_prompt_layout(name_lens: Sequence[int], n_ctx: int, L: int, position: str) -> torch.Tensor:
    """Source-row table [C, L] (int32) equivalent to the torch.cat's of forward_coop (trainers/mvlpt.py:439-515):
    0 = token_prefix, e > 0 = token_suffix[e-1], e < 0 = ctx[-e-1]."""
    rows = []
    for nl in name_lens:
        ctx = [-(j + 1) for j in range(n_ctx)]
        fixed = list(range(L - n_ctx))
        if n_ctx == 0:
            row = fixed
        elif position == "end":
            row = fixed[:1] + ctx + fixed[1:]
        elif position == "middle":
            half = n_ctx // 2
            row = fixed[:1] + ctx[:half] + fixed[1:1 + nl] + ctx[half:] + fixed[1 + nl:]
        elif position == "front":
            row = fixed[:1] + fixed[1:1 + nl] + ctx + fixed[1 + nl:]
        else:
            raise ValueError(position)
        if len(row) != L:
            raise ValueError("layout length mismatch")
        rows.append(row)
    return torch.tensor(rows, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ frozen CLIP
class FrozenCLIP:
    """What the reference passes around as ``clip_model``: here the frozen weights live packed inside the
    HIP engine; this object only carries what the prompt learner needs at construction time."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], compute_dtype: str = "fp16", device=None,
                 tokenizer=None, arch: Optional[ClipArch] = None, token_seed: int = 0, precision: str = "split_grad",
                 activation: str = "quick_gelu", vision_head_width: int = 64):
        # vision_head_width (MODEL.BACKBONE.VISION_HEAD_WIDTH): a state dict does not say it; ignored when `arch` is given
        self.arch = arch or arch_from_state_dict(state_dict, vision_head_width=vision_head_width)
        # activation: "quick_gelu" | "gelu" (MODEL.BACKBONE.ACTIVATION): what the checkpoint's MLPs were trained with
        self.engine = Engine.from_state_dict(state_dict, compute_dtype, device, self.arch, activation)
        self.engine.set_precision(precision)       # "fast" | "split_grad" | "split_all" (include/mvlpt_hip.h MVLPT_PREC_*)
        self.device = self.engine.device
        self.context_length = self.arch.context_length
        self.logit_scale = state_dict["logit_scale"].detach().float().to(self.device)     # frozen, clip/model.py:291
        self.tokenizer = tokenizer or default_tokenizer()
        self._token_embedding = state_dict.get("token_embedding.weight")
        self._token_seed = token_seed
        self._token_embedding_loaded = False      # the device copy encode_text needs (Engine.load_token_embedding), made on first use
        self.max_text_workspace_bytes = DEFAULT_MAX_TEXT_WORKSPACE_BYTES
        self.min_sequences_per_chunk = MIN_SEQUENCES_PER_CHUNK
        self.dtype = torch.float32   # dtype of the prompt parameters (see module docstring)
        # Engine.nearest_tokens: the same upload, on its first use (weak: the engine must not keep its owner alive in a cycle)
        self.engine.token_table_loader = weakref.WeakMethod(self._ensure_token_embedding)

    def _ensure_token_embedding(self) -> None:
        if not self._token_embedding_loaded:
            self.engine.load_token_embedding(self._token_table())
            self._token_embedding_loaded = True

    def token_embedding(self, ids: torch.Tensor) -> torch.Tensor:
        """clip_model.token_embedding(tokenized_prompts) (trainers/mvlpt.py:306-307); init-time only, CPU."""
        return self._token_table().float().cpu()[ids.cpu()]

    def _token_table(self) -> torch.Tensor:
        if self._token_embedding is None:
            self._token_embedding = _randn("token_embedding.weight", self._token_seed,
                                           (self.arch.vocab_size, self.arch.transformer_width), 0.02)
        return self._token_embedding

    # ------------------------------------------------------------------ clip_model.encode_text / encode_image
    def text_chunks(self, eot: Sequence[int], trim: bool = True):
        """The chunks encode_text runs for sequences with these EOT positions (plan_text_chunks on this engine's workspace sizes)."""
        return plan_text_chunks(eot, self.engine.text_encode_workspace_bytes, self.max_text_workspace_bytes,
                                min_chunk=self.min_sequences_per_chunk, force_len=None if trim else self.context_length)

    @torch.no_grad()
    def encode_text(self, tokenized, trim: bool = True) -> torch.Tensor:
        """clip_model.encode_text(tokenized) (clip/model.py:343-356): token ids [n, context_length] (a HOST tensor, as clip.tokenize
        returns) -> un-normalised features [n, embed] fp32 on the device, rows in input order.  The sequences are sorted by EOT
        position and run in chunks of their own length L = max eot + 1 (exact: the tower is causal, nothing behind the EOT token
        reaches the EOT row) whose workspace stays under `max_text_workspace_bytes`; trim = False runs every chunk at the full
        context length instead.  The first call uploads the token embedding (Engine.load_token_embedding)."""
        ids = torch.as_tensor(tokenized).cpu()
        if ids.dim() != 2 or ids.shape[0] == 0:
            raise ValueError("tokenized must be [n, context_length]")
        self._ensure_token_embedding()
        ids = ids.to(torch.int32).contiguous()
        chunks = self.text_chunks(ids.argmax(dim=-1).tolist(), trim)
        out = torch.empty(ids.shape[0], self.arch.embed_dim, device=self.device, dtype=torch.float32)
        for L, members in chunks:
            idx = torch.tensor(members, dtype=torch.long)
            feats = self.engine.text_encode_tokens(ids[idx], L)
            out.index_copy_(0, idx.to(self.device), feats)
        self.last_text_chunks = [(L, len(m)) for L, m in chunks]
        return out

    @torch.no_grad()
    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        """clip_model.encode_image(image) (clip/model.py:340-341): un-normalised features [B, embed] fp32."""
        return self.engine.image_fwd(image.to(self.device), None, None, save_for_bwd=False)


# Workspace budget of one encode_text chunk (not a reference key), the figure CoCoOp's tower uses
DEFAULT_MAX_TEXT_WORKSPACE_BYTES = 16 << 30
# sequences per tower: the attention launches put the sequence index on grid.y
MAX_SEQUENCES_PER_TOWER = 32768
# a bucket of equal-length sequences smaller than this takes the next lengths in as well (a tower over a handful of rows leaves the
# device idle; the positions it adds are bounded by min_chunk * (L_chunk - L_own))
MIN_SEQUENCES_PER_CHUNK = 512


def checkpoint_segments(layers: int, segments: int) -> List[tuple]:
    """TRAINER.ACT_CKPT's cut of the text blocks, [(first, last_exclusive, checkpointed)], by the rule of
    torch.utils.checkpoint.checkpoint_sequential (the reference: trainers/mvlpt.py:119-121): k = min(max(segments, 1), layers)
    segments, the first k - 1 of layers // k blocks each are checkpointed, the last one takes the rest and is saved.  The last
    segment is the largest and its size is not monotonic in k (12 layers: k = 5 -> 4 blocks, k = 7 -> 6).  The engine computes
    the same plan itself (Engine.text_act_ckpt_plan)."""
    k = min(max(int(segments), 1), int(layers))
    size = layers // k
    return [(i * size, (i + 1) * size, True) for i in range(k - 1)] + [((k - 1) * size, layers, False)]


def apply_text_act_ckpt(cfg, engine) -> int:
    """Set cfg.TRAINER.ACT_CKPT (absent: 1) on the engine of a model that is being built; returns the value.  The reference
    honours the key only together with CUT_CONTEXTLEN (its other branch calls self.transformer(x) directly); here it applies
    either way, since checkpointing changes no value.  An engine without the setting saves everything, which is ACT_CKPT = 1;
    asking such an engine for more is an error, not a silent no-op."""
    n = int(cfg.TRAINER.get("ACT_CKPT", 1))
    setter = getattr(engine, "set_text_act_ckpt", None)
    if setter is not None:
        setter(n)
    elif n != 1:
        raise ValueError(f"TRAINER.ACT_CKPT = {n}: this engine ({type(engine).__name__}) has no activation checkpointing")
    return n


def apply_text_grad_len(model, pl, classes: Optional[tuple] = None) -> None:
    """Tell the engine of `model` how far the next saving text forward's backward has to reach (Engine.set_text_grad_len): the largest
    EOT position of the class table of `pl` plus one, or every position when `model.text_grad_to_eot` is off
    (TRAINER.MVLPT.TEXT_GRAD_TO_EOT).  `classes` = (lo, hi): the class shard the tower runs, whose own maximum counts.  Called in
    front of every saving forward: several models may share one engine, and a class table may have been rebuilt since the last
    step.  A host call, nothing is enqueued; an engine without the setting runs every position."""
    setter = getattr(model.engine, "set_text_grad_len", None)
    if setter is None:
        return
    if classes is None:
        max_eot = int(pl.max_eot)
    else:      # (the shard's maximum is read back once per table: pl.eot lives on the device)
        key = (id(pl.eot), tuple(classes))
        if getattr(model, "_shard_max_eot", (None, 0))[0] != key:
            model._shard_max_eot = (key, int(pl.eot[classes[0]:classes[1]].max()))
        max_eot = model._shard_max_eot[1]
    full = int(model.clip_model.context_length)
    setter(min(max(max_eot + 1, TEXT_MIN_L), full) if getattr(model, "text_grad_to_eot", True) else full, max_eot)


def shared_prefix_len(layout: torch.Tensor, token_prefix: torch.Tensor, generic: bool, enabled: bool = True) -> int:
    """The leading positions every class prompt shares (Engine.set_text_shared_prefix): the leading columns of `layout` [C, L] that
    are identical in every class row and hold the prefix entry (0) or a context entry (< 0), never a suffix entry; 0 unless the
    context is generic, every row of `token_prefix` has the same bits and `enabled`.  Reads the tables back: cache the result."""
    if not enabled or not generic or layout.dim() != 2 or layout.shape[0] == 0:
        return 0
    rows = token_prefix.detach().reshape(token_prefix.shape[0], -1).contiguous().view(torch.uint8)      # bits, not values
    if rows.shape[0] != layout.shape[0] or not bool((rows == rows[:1]).all()):
        return 0
    ok = ((layout == layout[:1]).all(dim=0) & (layout[0] <= 0)).to("cpu")
    bad = (~ok).nonzero()
    return int(bad[0]) if bad.numel() else int(layout.shape[1])


def clamp_shared_prefix(prefix: int, seq_len: int, grad_len: int, min_len: int = TEXT_MIN_L) -> int:
    """The prefix the engine runs a tower of `seq_len` positions under, given the setting `prefix` and the gradient length: it fits
    a gradient slot (P <= grad_len - P) and leaves a slot `min_len` rows (the engine's rule, restated for planning and tests)."""
    p = min(int(prefix), seq_len - 1, grad_len // 2, grad_len - min_len)
    return max(p, 0)


# The shared prefix pays by the rows it removes, C * P - (L - P) of the forward's C * L (one slot of L - P rows is added), and costs
# one more launch per block in the backward (the reduction of the prefix keys' dK / dV), a serial link of the text chain: about
# 12 x 5 us at ViT-B's depth, the time of some 460 backward rows at the 0.13 us per row the gradient length measured
# (NOTES_experiments.md round 8).  An ESTIMATE, not a measured break-even (the kernel trace of round 9 has the reduce at 4.6 us
# alone and 36.6 us beside the image tower; no class table near the threshold was timed).  A class table that removes fewer rows than
# this runs every class in full, as it always did.
MIN_SHARED_PREFIX_ROWS = 512


def apply_text_shared_prefix(model, pl, layout: torch.Tensor, generic: bool, classes: Optional[tuple] = None) -> int:
    """Tell the engine of `model` how many leading positions the class prompts of the next text forward share
    (shared_prefix_len over the rows `classes` = (lo, hi) of `layout` / pl.token_prefix; TRAINER.MVLPT.TEXT_SHARED_PREFIX), or 0
    where that removes fewer than `model.shared_prefix_min_rows` (MIN_SHARED_PREFIX_ROWS) rows.  Called in front of every CoOp text
    forward, saving or not, next to apply_text_grad_len; the tables are read back once per class table.
    A host call; an engine without the setting evaluates every position of every class."""
    setter = getattr(model.engine, "set_text_shared_prefix", None)
    if setter is None:
        return 0
    enabled = bool(getattr(model, "text_shared_prefix", True))
    p = 0
    if enabled and generic:
        # (`layout` may be a trimmed view made for this call: the table it comes from identifies it, as in apply_text_grad_len)
        # (the tensors' version counters catch an in-place edit of a table)
        key = (id(pl.layout), id(pl.token_prefix), pl.layout._version, pl.token_prefix._version, tuple(layout.shape),
               tuple(classes) if classes is not None else None)
        if getattr(model, "_shared_prefix", (None, 0))[0] != key:
            lo, hi = classes if classes is not None else (0, layout.shape[0])
            model._shared_prefix = (key, shared_prefix_len(layout[lo:hi], pl.token_prefix[lo:hi], True))
        p = model._shared_prefix[1]
        n_cls = (classes[1] - classes[0]) if classes is not None else int(layout.shape[0])
        if n_cls * p - (int(layout.shape[1]) - p) < int(getattr(model, "shared_prefix_min_rows", MIN_SHARED_PREFIX_ROWS)):
            p = 0
    setter(min(p, int(model.clip_model.context_length) - 1))
    return p


def plan_text_chunks(eot: Sequence[int], workspace_bytes: Callable[[int, int], int], budget: int, min_len: int = TEXT_MIN_L,
                     max_seq: int = MAX_SEQUENCES_PER_TOWER, min_chunk: int = MIN_SEQUENCES_PER_CHUNK,
                     force_len: Optional[int] = None):
    """Cut sequences with EOT positions `eot` into towers: [(L, [indices into eot])].  Pure host arithmetic.
    The sequences are sorted by EOT position (ties by index).  A chunk starts at the shortest sequence not yet placed, takes every
    sequence of that length, and goes on into longer ones only while it holds fewer than `min_chunk`; it never holds more than
    `max_seq` sequences and `workspace_bytes(count, L)` never exceeds `budget`, with L = the longest member's eot + 1, raised to
    `min_len` (force_len: that length for every chunk).  Chunks are returned largest workspace first, so that a grow-only workspace
    is sized once.  Raises ValueError when a single sequence does not fit the budget."""
    eot = [int(v) for v in eot]
    if any(v < 0 for v in eot):
        raise ValueError("EOT positions must be >= 0")
    order = sorted(range(len(eot)), key=lambda i: (eot[i], i))

    def length(i):
        return force_len if force_len is not None else max(eot[i] + 1, min_len)

    if force_len is not None and order and eot[order[-1]] >= force_len:
        raise ValueError(f"an EOT position lies outside the forced length {force_len}")
    chunks, a, n = [], 0, len(order)
    while a < n:
        if workspace_bytes(1, length(order[a])) > budget:
            raise ValueError(f"one sequence of length {length(order[a])} needs {workspace_bytes(1, length(order[a]))} bytes of text "
                             f"workspace, over the budget of {budget}")
        b = a + 1
        while b < n and b - a < max_seq:
            same = length(order[b]) == length(order[b - 1])
            if not same and b - a >= min_chunk:
                break
            if workspace_bytes(b - a + 1, length(order[b])) > budget:
                break
            b += 1
        chunks.append((length(order[b - 1]), order[a:b]))
        a = b
    chunks.sort(key=lambda c: -workspace_bytes(len(c[1]), c[0]))
    return chunks


# ------------------------------------------------------------------------------------------------ UPT projection
class _ProjAttention(nn.Module):
    """Parameter container with nn.MultiheadAttention's names (in_proj_weight, in_proj_bias, out_proj.*)."""

    def __init__(self, d: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = nn.Linear(d, d)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class _ProjBlock(nn.Module):
    """clip.model.ResidualAttentionBlock(width, heads=1) as the reference USES it in forward_mvlpt_proj
    (trainers/mvlpt.py:403-407): a batch-first [1,T,D] tensor goes into a seq-first block, so attention sees
    sequence length 1 and the softmax over the single key is 1:
        x + out_proj(v_proj(ln_1(x)));  then  + c_proj(QuickGELU(c_fc(ln_2(.))))."""

    def __init__(self, d: int):
        super().__init__()
        self.attn = _ProjAttention(d)
        self.ln_1 = nn.LayerNorm(d)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d, 4 * d)), ("gelu", nn.Identity()),
                                              ("c_proj", nn.Linear(4 * d, d))]))
        self.ln_2 = nn.LayerNorm(d)

    def forward(self, x):
        d = x.shape[-1]
        wv, bv = self.attn.in_proj_weight[2 * d:], self.attn.in_proj_bias[2 * d:]
        x = x + self.attn.out_proj(nn.functional.linear(self.ln_1(x), wv, bv))
        u = self.mlp.c_fc(self.ln_2(x))
        return x + self.mlp.c_proj(u * torch.sigmoid(1.702 * u))


class _ProjTransformer(nn.Module):
    def __init__(self, width: int):
        super().__init__()
        self.width, self.layers = width, 1
        self.resblocks = nn.Sequential(_ProjBlock(width))

    def forward(self, x):
        return self.resblocks(x)


# ------------------------------------------------------------------------------------------------ prompt learner
def class_prompt_tables(clip_model: FrozenCLIP, classnames, pretokenized: Optional[PretokenizedPrompts], prompt_prefix: str, cut: bool):
    """Tokenisation + frozen token embeddings of the class prompts (init time, CPU; trainers/mvlpt.py:292-307, trainers/cocoop.py:105-111):
    (tokenized_prompts [n_cls, L], name_lens, embedding [n_cls, L, ctx_dim]).  `pretokenized` gives the first two instead of the
    tokenizer; `cut` is TRAINER.CUT_CONTEXTLEN (L = the longest prompt), which the reference's CoCoOp trainer does not have."""
    if pretokenized is not None:
        tokenized_prompts, name_lens = pretokenized.tokenized_prompts, pretokenized.name_lens
    else:
        tok = clip_model.tokenizer
        names = [n.replace("_", " ") for n in classnames]
        name_lens = [len(tok.encode(n)) for n in names]
        prompts = [prompt_prefix + " " + n + "." for n in names]
        max_length = clip_model.context_length
        if cut:
            max_length = min(max_length, max(len(tok.encode(p)) + 2 for p in prompts))
        tokenized_prompts = torch.cat([tok.tokenize(p, context_length=max_length) for p in prompts])
    with torch.no_grad():
        embedding = clip_model.token_embedding(tokenized_prompts).to(clip_model.dtype)
    return tokenized_prompts, name_lens, embedding


def register_class_tables(pl: nn.Module, n_cls: int, tables, n_ctx: int, position: str) -> None:
    """Give the prompt learner `pl` what the HIP text tower reads, from `class_prompt_tables`: the `token_prefix` / `token_suffix`
    buffers (saved by save_model, dropped by load_model; :312-316), the integer tables `layout` and `eot` (not persistent), and
    `n_cls`, `tokenized_prompts`, `name_lens`, `max_eot`.  `n_ctx` context tokens stand at `position` ("end" | "middle" | "front")."""
    tokenized_prompts, name_lens, embedding = tables
    pl.register_buffer("token_prefix", embedding[:, :1, :].contiguous())                # SOS
    pl.register_buffer("token_suffix", embedding[:, 1 + n_ctx:, :].contiguous())        # CLS, EOS
    pl.n_cls = n_cls
    pl.tokenized_prompts = tokenized_prompts
    pl.name_lens = list(name_lens)
    L = tokenized_prompts.shape[1]
    pl.register_buffer("layout", build_prompt_layout(pl.name_lens, n_ctx, L, position), persistent=False)
    pl.register_buffer("eot", tokenized_prompts.argmax(dim=-1).to(torch.int32), persistent=False)   # :128
    pl.max_eot = int(pl.eot.max())


def image_conditioned_ctx(clip_model: FrozenCLIP, n_ctx: int, ctx_init: str, ctx_dim: int, vis_dim: int, dtype):
    """CoCoOp's trainable text side (trainers/cocoop.py:76-100, trainers/mvlpt.py:262-286): the context vectors [n_ctx, ctx_dim] (the
    embedding of `ctx_init`, or N(0, 0.02)) and then `meta_net`, in the order the RNG is consumed.  Returns (ctx_vectors, meta_net,
    prompt_prefix, n_ctx): `ctx_init` sets its own n_ctx."""
    if ctx_init:
        ctx_init = ctx_init.replace("_", " ")
        n_ctx = len(ctx_init.split(" "))
        ids = clip_model.tokenizer.tokenize(ctx_init)
        with torch.no_grad():
            ctx_vectors = clip_model.token_embedding(ids)[0, 1:1 + n_ctx, :].to(dtype)
        prompt_prefix = ctx_init
    else:
        ctx_vectors = torch.empty(n_ctx, ctx_dim, dtype=dtype)
        nn.init.normal_(ctx_vectors, std=0.02)
        prompt_prefix = " ".join(["X"] * n_ctx)
    meta_net = nn.Sequential(OrderedDict([
        ("linear1", nn.Linear(vis_dim, vis_dim // 16)),
        ("relu", nn.ReLU(inplace=True)),
        ("linear2", nn.Linear(vis_dim // 16, ctx_dim)),
    ]))
    return ctx_vectors, meta_net, prompt_prefix, n_ctx


def deep_text_prompts(cfg, arch: ClipArch) -> int:
    """TRAINER.MVLPT.COOP.N_DEEP (absent: 0) of a model that is being built, checked against everything the deep text route does not
    offer; every refusal names its cause and comes before anything is allocated.  Deep language prompting replaces the hidden states
    at the context positions in front of text blocks 1 .. N_DEEP by the rows of `ctx_deep` [N_DEEP, n_ctx, width]."""
    T = cfg.TRAINER.MVLPT
    n_deep = int(T.COOP.get("N_DEEP", 0))
    if n_deep == 0:
        return 0
    if n_deep < 0:
        raise ValueError(f"COOP.N_DEEP = {n_deep}: the number of deep text prompt layers cannot be negative")
    if T.COCOOP.N_CTX != 0:
        raise NotImplementedError("COOP.N_DEEP > 0 together with COCOOP.N_CTX != 0: the image-conditioned (ranged) text tower has no "
                                  "deep prompts; set COCOOP.N_CTX 0")
    if T.COOP.N_CTX == 0:
        raise ValueError("COOP.N_DEEP > 0 needs context tokens: the deep prompts replace the hidden states at the context positions, "
                         "and COOP.N_CTX is 0")
    if T.COOP.CSC:
        raise NotImplementedError("COOP.N_DEEP > 0 together with COOP.CSC: per-class deep prompts are not offered (the deep rows are "
                                  "shared by all classes); set COOP.CSC False")
    if n_deep > arch.transformer_layers - 1:
        raise ValueError(f"COOP.N_DEEP = {n_deep} exceeds transformer_layers - 1 = {arch.transformer_layers - 1}: block 0 reads the "
                         "embedding-level context `ctx`, only the later blocks take deep prompts")
    if T.VPT.N_CTX != 0 and T.PROJECT_METHOD != "identity":
        raise NotImplementedError(f"COOP.N_DEEP > 0 with visual prompts under PROJECT_METHOD = {T.PROJECT_METHOD!r}: the UPT projection "
                                  "has no place for the deep text prompts; set PROJECT_METHOD \"identity\" (independent V-L prompting)")
    return n_deep


class MultitaskVLPromptLearner(nn.Module):
    """trainers/mvlpt.py:138-515.  ``clip_model`` is a :class:`FrozenCLIP`; ``classnames`` a list of str, or a
    :class:`PretokenizedPrompts` (then ``classnames`` only gives n_cls)."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        n_cls = len(classnames)
        T = cfg.TRAINER.MVLPT
        coop_n_ctx, cocoop_n_ctx, vpt_n_ctx = T.COOP.N_CTX, T.COCOOP.N_CTX, T.VPT.N_CTX
        n_deep = deep_text_prompts(cfg, clip_model.arch)
        if cocoop_n_ctx != 0:
            raise NotImplementedError("COCOOP.N_CTX != 0 is not this class's route: image-conditioned prompts live in "
                                      "mvlpt_amd.mvlpt_cocoop (MultitaskVLPromptLearner / CustomCLIP there; MVLPT.build_model picks them)")
        arch = clip_model.arch
        dtype = clip_model.dtype
        coop_ctx_dim, vpt_ctx_dim = arch.transformer_width, arch.vision_width
        self._init_visual_prompts(cfg, clip_model)
        prompt_prefix = "a photo of a " if vpt_n_ctx != 0 else ""                       # :201

        self.ctx = None
        if coop_n_ctx != 0:
            if T.COOP.CTX_INIT:
                init = T.COOP.CTX_INIT.replace("_", " ")
                coop_n_ctx = len(init.split(" "))
                ids = clip_model.tokenizer.tokenize(init)
                ctx_vectors = clip_model.token_embedding(ids)[0, 1:1 + coop_n_ctx, :].to(dtype)   # :208-216
                prompt_prefix = init
            else:
                shape = (n_cls, coop_n_ctx, coop_ctx_dim) if T.COOP.CSC else (coop_n_ctx, coop_ctx_dim)
                ctx_vectors = torch.empty(*shape, dtype=dtype)
                nn.init.normal_(ctx_vectors, std=0.02)                                  # :220-226
                prompt_prefix = " ".join(["X"] * coop_n_ctx)
            self.ctx = nn.Parameter(ctx_vectors)

        self.mvlpt_proj = nn.Identity()
        if vpt_n_ctx != 0 and coop_n_ctx != 0:
            self.mvlpt_proj_ctx_dim = T.PROJECT_DIM
            if T.PROJECT_METHOD == "identity":
                self.mvlpt_proj = nn.Identity()
            else:
                self.mvlpt_proj_ctx_vpt_pre, self.mvlpt_proj_ctx_vpt_post = nn.Identity(), nn.Identity()
                self.mvlpt_proj_ctx_coop_pre, self.mvlpt_proj_ctx_coop_post = nn.Identity(), nn.Identity()
                D = self.mvlpt_proj_ctx_dim
                if coop_ctx_dim != D:
                    self.mvlpt_proj_ctx_coop_pre = nn.Linear(coop_ctx_dim, D, dtype=dtype)
                    self.mvlpt_proj_ctx_coop_post = nn.Linear(D, coop_ctx_dim, dtype=dtype)
                if vpt_ctx_dim != D:
                    self.mvlpt_proj_ctx_vpt_pre = nn.Linear(vpt_ctx_dim, D, dtype=dtype)
                    self.mvlpt_proj_ctx_vpt_post = nn.Linear(D, vpt_ctx_dim, dtype=dtype)
                if T.PROJECT_METHOD == "transformer":
                    self.mvlpt_proj = _ProjTransformer(D)
                else:
                    # 'mlp' crashes in the reference too (nn.GeLU, trainers/mvlpt.py:253)
                    raise AttributeError("module 'torch.nn' has no attribute 'GeLU'")
        self.cocoop_ctx = None
        # deep text prompts (COOP.N_DEEP; not in the reference): drawn after every other draw, so a seed gives the same ctx / vpt_*
        # with and without them; the attribute exists only with N_DEEP > 0, so the state_dict keys are unchanged at 0
        self.coop_n_deep = n_deep
        if n_deep > 0:
            ctx_deep = torch.empty(n_deep, coop_n_ctx, coop_ctx_dim, dtype=dtype)
            nn.init.normal_(ctx_deep, std=0.02)
            self.ctx_deep = nn.Parameter(ctx_deep)

        self.vpt_n_ctx, self.coop_n_ctx, self.cocoop_n_ctx = vpt_n_ctx, coop_n_ctx, 0
        self.class_token_position = T.COOP.CLASS_TOKEN_POSITION
        tables = class_prompt_tables(clip_model, classnames, pretokenized, prompt_prefix, cfg.TRAINER.CUT_CONTEXTLEN)
        register_class_tables(self, n_cls, tables, coop_n_ctx, self.class_token_position)

    def _init_visual_prompts(self, cfg, clip_model: FrozenCLIP) -> None:
        """The image side of the constructor (trainers/mvlpt.py:165-201), for this class and the COCOOP.N_CTX != 0 route: the ResNet
        refusal, the image-size check, `vpt_dropout` / `vpt_deep`, and with VPT.N_CTX != 0 `vpt_proj`, `vpt_embeddings` and
        `vpt_embeddings_deep` (None otherwise).  The RNG is consumed in that order."""
        V = cfg.TRAINER.MVLPT.VPT
        arch, dtype = clip_model.arch, clip_model.dtype
        vpt_n_ctx, vpt_ctx_dim = V.N_CTX, arch.vision_width
        if is_resnet(arch) and vpt_n_ctx != 0:
            raise ValueError("visual prompts (VPT.N_CTX != 0, UPT) need a ViT backbone: a ResNet tower is frozen and forward-only here, and the "
                             "reference cannot prompt it either (trainers/mvlpt.py:48 \"HACK: Assume all is vision transformer\")")
        clip_imsize, cfg_imsize = arch.image_resolution, cfg.INPUT.SIZE[0]
        assert cfg_imsize == clip_imsize, f"cfg_imsize ({cfg_imsize}) must equal to clip_imsize ({clip_imsize})"

        self.vpt_dropout = nn.Dropout(V.DROPOUT)                                        # :165 (applied per image: CustomCLIP.forward)
        self.vpt_deep = V.DEEP
        self.vpt_embeddings = None
        self.vpt_embeddings_deep = None
        if vpt_n_ctx == 0:
            return
        if V.PROJECT > -1:                                                              # :170-175
            vpt_dim = V.PROJECT
            self.vpt_proj = nn.Linear(vpt_dim, vpt_ctx_dim, dtype=dtype)
            nn.init.kaiming_normal_(self.vpt_proj.weight, a=0, mode="fan_out")
        else:
            vpt_dim = vpt_ctx_dim
            self.vpt_proj = nn.Identity()
        if V.CTX_INIT:
            raise ValueError("CTX initiation scheme is not supported")                # :180-182
        ps = arch.vision_patch_size
        val = math.sqrt(6. / float(3 * reduce(mul, (ps, ps), 1) + vpt_dim))             # :186
        self.vpt_embeddings = nn.Parameter(torch.zeros(1, vpt_n_ctx, vpt_dim, dtype=dtype))
        nn.init.uniform_(self.vpt_embeddings.data, -val, val)
        if self.vpt_deep:
            self.vision_layers = arch.vision_layers
            self.vpt_embeddings_deep = nn.Parameter(torch.zeros(arch.vision_layers - 1, vpt_n_ctx, vpt_dim, dtype=dtype))
            nn.init.uniform_(self.vpt_embeddings_deep.data, -val, val)

    # trainers/mvlpt.py:376-414
    def forward_mvlpt_proj(self, dtype=torch.float):
        if self.coop_n_ctx == 0 or isinstance(self.mvlpt_proj, nn.Identity) or self.vpt_n_ctx == 0:
            return self.ctx, self.vpt_embeddings, self.vpt_embeddings_deep
        vpt_emb = self.vpt_embeddings
        if self.vpt_deep:
            vpt_emb = torch.cat([vpt_emb, self.vpt_embeddings_deep], dim=0)
        vpt_ctx_dim = vpt_emb.shape[-1]
        vpt_emb = vpt_emb.reshape(1, -1, vpt_ctx_dim)
        coop_emb = self.ctx
        coop_ctx_dim = self.ctx.shape[-1]
        if coop_emb.dim() == 2:
            coop_emb = coop_emb.unsqueeze(0)
        coop_emb = coop_emb.reshape(1, -1, coop_ctx_dim)
        n = coop_emb.shape[1]
        coop_emb = self.mvlpt_proj_ctx_coop_pre(coop_emb)
        vpt_emb = self.mvlpt_proj_ctx_vpt_pre(vpt_emb)
        e = self.mvlpt_proj(torch.cat([coop_emb, vpt_emb], dim=1).float()).type(dtype)
        coop_emb, vpt_emb = e[:, :n, :], e[:, n:, :]
        coop_emb = self.mvlpt_proj_ctx_coop_post(coop_emb).reshape(-1, self.coop_n_ctx, coop_ctx_dim).squeeze(0)
        vpt_emb = self.mvlpt_proj_ctx_vpt_post(vpt_emb).reshape(-1, self.vpt_n_ctx, vpt_ctx_dim)
        vpt_emb_deep = None if vpt_emb.shape[0] == 1 else vpt_emb[1:, :, :]
        return coop_emb, vpt_emb[0, :, :].unsqueeze(0), vpt_emb_deep


# ------------------------------------------------------------------------------------------------ class sharding
def class_shard_bounds(n_cls: int, world: int):
    """Balanced contiguous split of the classes over the ranks: the first n_cls % world ranks own one class more."""
    base, rem = divmod(n_cls, world)
    return [(r * base + min(r, rem), (r + 1) * base + min(r + 1, rem)) for r in range(world)]


class ClassShard:
    """Class-sharded text tower (collective 2): rank r encodes classes bounds[r] only.  Every rank contributes
    a slot of `cmax` rows (the largest shard) to ONE all_gather_into_tensor of the features and receives its slot of ONE
    reduce_scatter_tensor (sum) of their gradients, both on persistent buffers.  Shards of equal size need no other launch
    (the gathered buffer IS the [n_cls, e] feature matrix); ragged shards (n_cls % world != 0) add one index_select /
    index_copy with index tensors built once.  Per step N > 1 adds: 1 copy + 1 all-gather (+1), 1 reduce-scatter (+1)."""

    def __init__(self, rank: int, bounds, device, dtype=torch.float32):
        self.rank, self.bounds, self.world = rank, bounds, len(bounds)
        self.cmax = max(hi - lo for lo, hi in bounds)
        self.lo, self.hi = bounds[rank]
        self.even = all(hi - lo == self.cmax for lo, hi in bounds)
        self.device, self.dtype = device, dtype
        self._e = None
        # slot row of every class (class c of rank r sits at r * cmax + (c - lo_r))
        self.slot_of_class = torch.cat([torch.arange(hi - lo) + r * self.cmax for r, (lo, hi) in enumerate(bounds)]).to(device)

    def _buffers(self, e: int):
        if self._e != e:
            z = lambda rows: torch.zeros(rows, e, device=self.device, dtype=self.dtype)
            self.gin, self.gout, self.sin, self.sout = z(self.cmax), z(self.world * self.cmax), z(self.world * self.cmax), z(self.cmax)
            self._e = e
        return self.gin, self.gout, self.sin, self.sout

    def gather(self, loc: torch.Tensor) -> torch.Tensor:
        """per-rank text features [c_r, e] -> [n_cls, e] on every rank (RCCL over xGMI: <= 4.5 MB)."""
        import torch.distributed as dist
        gin, gout, _, _ = self._buffers(loc.shape[1])
        gin[:loc.shape[0]].copy_(loc)                     # pad rows (ragged shards) stay zero
        if dist.get_backend() == "gloo":                  # CPU tests / one-GPU debug mode: host-staged, disjoint slots summed
            h = torch.zeros(gout.shape, dtype=gout.dtype)
            h[self.rank * self.cmax:(self.rank + 1) * self.cmax] = gin.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            gout.copy_(h)
        else:
            dist.all_gather_into_tensor(gout, gin)
        return gout if self.even else gout.index_select(0, self.slot_of_class)

    def scatter_grads(self, dtxt: torch.Tensor) -> torch.Tensor:
        """reduce-scatter (sum over ranks) of d txt [n_cls, e] back to the class owners -> [hi - lo, e]."""
        import torch.distributed as dist
        _, _, sin, sout = self._buffers(dtxt.shape[1])
        if self.even:
            src = dtxt.contiguous()
        else:
            sin.index_copy_(0, self.slot_of_class, dtxt)  # pad rows were zeroed at allocation and are never written
            src = sin
        if dist.get_backend() == "gloo":                  # gloo has no reduce_scatter: host-staged all-reduce
            h = src.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            sout.copy_(h[self.rank * self.cmax:(self.rank + 1) * self.cmax])
        else:
            dist.reduce_scatter_tensor(sout, src, op=dist.ReduceOp.SUM)
        return sout[:self.hi - self.lo]


# ------------------------------------------------------------------------------------------------ autograd bridge
def _text_inputs(model, pl, n_ctx):
    """token_suffix / layout handed to the text tower, for a prompt learner `pl` with `n_ctx` context tokens.
    With `trim_text_to_eot` (off by default) only the first max(eot)+1 positions are evaluated: the text transformer is causal (clip/model.py:324-330) and the feature is read
    at the EOT position (trainers/mvlpt.py:128), so later (padding) positions can influence neither the logits nor
    any gradient — the same observation the reference's CUT_CONTEXTLEN option is built on (trainers/mvlpt.py:297-305)."""
    if not model.trim_text_to_eot:
        return pl.token_suffix, pl.layout
    L_eff = pl.max_eot + 1
    return pl.token_suffix[:, :L_eff - 1 - n_ctx], pl.layout[:, :L_eff]


class _PromptedClipFn(torch.autograd.Function):
    """CustomCLIP.forward as ONE autograd node: forward and backward are libmvlpt_hip.so calls."""

    @staticmethod
    def forward(fctx, model: "CustomCLIP", image, task_lo, task_hi, coop_emb, vpt_emb, vpt_deep_emb, grad_on=True, ctx_deep=None):
        eng = model.engine
        pl = model.prompt_learner
        # (grad mode is off inside Function.forward: ask autograd which inputs need a gradient)
        # `grad_on` = torch.is_grad_enabled() at the call site (needs_input_grad ignores torch.no_grad())
        need_txt = grad_on and bool(fctx.needs_input_grad[4] or fctx.needs_input_grad[8])
        need_img = grad_on and bool(fctx.needs_input_grad[5] or fctx.needs_input_grad[6])

        # 1. text features from the cache, or a text job to run
        txt, slot = model.text_cache.lookup(pl, coop_emb is not None, need_txt)
        shard = text_job = None
        if txt is None:
            suffix, layout = _text_inputs(model, pl, pl.coop_n_ctx)
            shard = model._class_shard if coop_emb is not None else None
            if need_txt:
                apply_text_grad_len(model, pl, (shard.lo, shard.hi) if shard is not None else None)
            # the leading positions every class shares are evaluated once (generic context, no deep prompts; saving or not)
            apply_text_shared_prefix(model, pl, layout, coop_emb is not None and coop_emb.dim() == 2 and ctx_deep is None,
                                     (shard.lo, shard.hi) if shard is not None else None)
            if shard is not None:
                # Class-sharded text tower (ClassShard): this rank encodes classes [lo, hi) only and the features are
                # all-gathered; the backward reduce-scatters d(txt) back to the owners.  Tower and collective are one job.
                lo, hi = shard.lo, shard.hi
                ctx_loc = coop_emb if coop_emb.dim() == 2 else coop_emb[lo:hi]

                def text_job():
                    loc = eng.text_fwd(pl.token_prefix[lo:hi], suffix[lo:hi], ctx_loc, layout[lo:hi], pl.eot[lo:hi],
                                       save_for_bwd=need_txt)
                    return shard.gather(loc)
            elif ctx_deep is not None:
                # deep text prompts (COOP.N_DEEP): the same tower through the deep entries; class sharding is refused at set-up
                def text_job():
                    return eng.text_fwd_deep(pl.token_prefix, suffix, coop_emb, ctx_deep, layout, pl.eot, save_for_bwd=need_txt)
            else:
                def text_job():
                    return eng.text_fwd(pl.token_prefix, suffix, coop_emb, layout, pl.eot, save_for_bwd=need_txt)

        # 2. image features from the prefetch (prefetch_image_features), or an image job to run
        entry = model.prefetch.claim(image, prompted=vpt_emb is not None)

        def image_job():
            if entry is not None:
                return model.prefetch.pick_up(entry)
            return eng.image_fwd(image, vpt_emb, vpt_deep_emb, save_for_bwd=need_img)

        # 3. The two towers are independent until the logits: the text tower (few, small launches that cannot fill 256 CUs) is
        # forked onto the text stream underneath the image tower's large GEMMs and joined behind it.  With no such stream the
        # "join" is the text job itself: inline, image tower first, then text
        side = model.text_stream if (text_job is not None and model.overlap_towers) else None
        join = text_job if side is None else fork(side, text_job)
        img = image_job()
        if text_job is not None:
            txt = join()
            model.text_cache.store(slot, txt, gathered=shard is not None)

        # 4. the head
        logits = eng.logits_fwd(img, txt, model.logit_scale_exp, task_lo, task_hi)
        model._fwd_generation += 1               # (check_forward_is_current)
        fctx.generation = model._fwd_generation
        fctx.model, fctx.need_img, fctx.need_txt = model, need_img, need_txt
        fctx.shard, fctx.ctx_shape = shard, (None if coop_emb is None else coop_emb.shape)
        fctx.text_deep = ctx_deep is not None
        fctx.vpt_shape = None if vpt_emb is None else vpt_emb.shape
        return logits

    @staticmethod
    def backward(fctx, dlogits):
        model, shard = fctx.model, fctx.shard
        eng = model.engine
        check_forward_is_current(model, fctx.generation)
        dimg, dtxt = eng.logits_bwd(dlogits.contiguous(), fctx.need_img, fctx.need_txt)
        dctx = dvpt = ddeep = dctx_deep = None
        if fctx.need_txt:
            if shard is not None:
                def text_job():
                    # sum over ranks of d(local loss)/d(txt) for the classes this rank owns; the trainer's gradient
                    # all-reduce (mean over ranks) then yields d(global mean loss)/d(ctx) summed over all class shards
                    own = shard.scatter_grads(dtxt)
                    dloc = eng.text_bwd(own)
                    if len(fctx.ctx_shape) == 3:                      # class-specific contexts: only the owned rows are non-zero
                        full = torch.zeros(fctx.ctx_shape, device=dloc.device, dtype=dloc.dtype)
                        full[shard.lo:shard.hi] = dloc
                        return full, None
                    return dloc, None
            elif fctx.text_deep:
                def text_job():
                    return eng.text_bwd_deep(dtxt)
            else:
                def text_job():
                    return eng.text_bwd(dtxt), None
            # CU partition (set_cu_partition): the backward of the text tower stays on the text stream's compute units,
            # next to the image tower of the following batch on the prefetch stream's; otherwise it runs where it is
            partitioned = model.text_cus and shard is None and not fctx.need_img
            join = fork(model.text_stream, text_job, uses=(dtxt,)) if partitioned else text_job
            dctx, dctx_deep = join()
        if fctx.need_img:
            dvpt, ddeep = eng.image_bwd(dimg)
            dvpt = dvpt.view(fctx.vpt_shape)
        return None, None, None, None, dctx, dvpt, ddeep, None, dctx_deep


class _CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy (mean) with the gradient produced by the same fused HIP kernel."""

    @staticmethod
    def forward(fctx, model, logits, label):
        loss, dl, nc = model.engine.cross_entropy(logits, label, need_grad=bool(fctx.needs_input_grad[1]))
        if dl is not None:
            fctx.save_for_backward(dl)
        model.last_ncorrect = nc
        return loss.squeeze(0)

    @staticmethod
    def backward(fctx, g):
        (dl,) = fctx.saved_tensors
        return None, dl * g, None


def class_range_tables(dm):
    """(start, end): the class range of every task, indexed by task id; sized num_classes as in the reference
    (trainers/mvlpt.py:529-537).  Host tensors."""
    start = torch.arange(dm._num_classes)
    end = torch.arange(dm._num_classes)
    s = 0
    for i, task in enumerate(dm._task_names):
        start[i] = s
        s += len(dm._labelmap[task])
        end[i] = s
    return start, end


class VisualPromptSide:
    """The visual-prompt side of a model with a `prompt_learner` of MultitaskVLPromptLearner's kind, `engine`, `clip_model` and
    `dtype`: mvlpt_amd.model.CustomCLIP and mvlpt_amd.mvlpt_cocoop.CustomCLIP."""

    def projected_prompts(self, batch: Optional[int] = None):
        """(coop_emb, vpt, vpt_deep) as the towers take them: forward_mvlpt_proj, then vpt_proj (VPT.PROJECT > -1: a trainable
        Linear, else Identity) in front of the shallow and of every deep prompt (:424, :77) — a few hundred FLOPs on [n, vpt_dim]
        rows, left to torch autograd.  `batch`: the forward over that many images follows, and the engine gets its dropout masks."""
        pl = self.prompt_learner
        coop_emb, vpt_emb, vpt_emb_deep = pl.forward_mvlpt_proj(self.dtype)
        if vpt_emb is not None:
            vpt_emb = pl.vpt_proj(vpt_emb)
            if vpt_emb_deep is not None:
                vpt_emb_deep = pl.vpt_proj(vpt_emb_deep)
            if batch is not None:
                self.engine.set_vpt_dropout(self.vpt_dropout_masks(batch))
        return coop_emb, vpt_emb, vpt_emb_deep

    def vpt_dropout_masks(self, B):
        """Outcome of `vpt_dropout` on the prompt rows of every prompted layer, drawn in the reference's order (the shallow prompts
        in forward_vpt, trainers/mvlpt.py:424, then layer 1, 2, ... in ImageEncoder.forward, :77), each on the rows already expanded
        over the batch: [n_layers, B, n_vpt, width] of 0 or 1 / (1 - p), or None when nothing is dropped (p = 0, eval mode)."""
        pl = self.prompt_learner
        p = float(pl.vpt_dropout.p)
        if pl.vpt_embeddings is None or p == 0.0 or not pl.training:
            return None
        if getattr(self, "_vpt_masks_override", None) is not None:      # tests: the masks the reference drew
            return self._vpt_masks_override
        n_layers = 1 + (pl.vpt_embeddings_deep.shape[0] if (pl.vpt_deep and pl.vpt_embeddings_deep is not None) else 0)
        dev = pl.vpt_embeddings.device
        ones = torch.ones(B, pl.vpt_n_ctx, self.clip_model.arch.vision_width, device=dev)
        return torch.stack([pl.vpt_dropout(ones) for _ in range(n_layers)])


class CustomCLIP(VisualPromptSide, nn.Module):
    """trainers/mvlpt.py:517-583.  The step schedule (mvlpt_amd.schedule, DESIGN.md "Step schedule"): `text_stream` carries the text
    tower beside the image tower when `overlap_towers`, `prefetch` the image towers computed ahead, `text_cache` the text features
    that outlive a forward."""

    def __init__(self, cfg, classnames, clip_model: FrozenCLIP, dm=None, pretokenized: Optional[PretokenizedPrompts] = None):
        super().__init__()
        self.prompt_learner = MultitaskVLPromptLearner(cfg, classnames, clip_model, pretokenized)
        self.tokenized_prompts = self.prompt_learner.tokenized_prompts
        self.clip_model = clip_model
        self.engine = clip_model.engine
        self.text_act_ckpt = apply_text_act_ckpt(cfg, self.engine)      # TRAINER.ACT_CKPT
        self.logit_scale = clip_model.logit_scale
        self.logit_scale_exp = float(clip_model.logit_scale.exp())
        self.dtype = clip_model.dtype
        self.last_ncorrect = None
        self.overlap_towers = True
        self._class_shard = None
        self.trim_text_to_eot = False
        self.text_grad_to_eot = bool(cfg.TRAINER.MVLPT.get("TEXT_GRAD_TO_EOT", True))
        self.text_shared_prefix = bool(cfg.TRAINER.MVLPT.get("TEXT_SHARED_PREFIX", True))
        self.shared_prefix_min_rows = MIN_SHARED_PREFIX_ROWS
        self.text_cache = TextFeatureCache()
        self.prefetch = ImagePrefetch(self.engine, clip_model.device)
        self._fwd_generation = 0
        # None without a GPU: both towers inline.  Under a CU partition (text_cus > 0) it owns compute units [0, text_cus)
        self.text_stream = torch.cuda.Stream(device=clip_model.device) if torch.cuda.is_available() else None
        self.text_cus = 0
        if self.text_stream is not None:
            self.set_cu_partition(int(os.environ.get("MVLPT_TEXT_CUS", DEFAULT_TEXT_CUS)))
        self.multi_task_label_pertask = cfg.DATASET.MULTITASK_LABEL_PERTASK
        if self.multi_task_label_pertask:
            self.class_index_pertask_start, self.class_index_pertask_end = class_range_tables(dm)

    def enable_class_sharding(self, rank: int, world: int) -> None:
        """Shard the text tower over classes across `world` data-parallel ranks (many-class configs: the text tower
        costs C * L tokens per step independent of the batch, so replicating it caps weak scaling)."""
        if world <= 1:
            self._class_shard = None
            return
        if getattr(self.prompt_learner, "coop_n_deep", 0) > 0:
            raise NotImplementedError("class sharding with deep text prompts (COOP.N_DEEP > 0) is not offered: the sharded text tower "
                                      "runs the plain entries; set COOP.N_DEEP 0 or run the text tower replicated")
        C = self.prompt_learner.n_cls
        if world > C:
            raise ValueError(f"class sharding needs at least one class per rank ({C} classes, {world} ranks)")
        self._class_shard = ClassShard(rank, class_shard_bounds(C, world), self.clip_model.device)

    def set_cu_partition(self, text_cus: int) -> None:
        """Run the two towers on disjoint compute units (methods without visual prompts, i.e. the cross-step pipeline of
        prefetch_image_features): the text tower forward AND backward on a stream that owns logical CUs [0, text_cus), the
        image tower of the following batch on a stream that owns the rest (include/mvlpt_hip.h: mvlpt_stream_create_cus).
        Without it the image tower's persistent GEMM workgroups hold every CU for a whole launch and the text tower's short
        kernels only run in their tails (measured: each stretches ~3x, only 1.7 of 4.4 ms hide).  0 switches it off."""
        from .engine import device_cus, partition_stream
        dev = self.clip_model.device
        pl = self.prompt_learner
        if text_cus <= 0 or pl.vpt_embeddings is not None or pl.coop_n_ctx == 0:
            if self.text_cus:
                self.text_stream = torch.cuda.Stream(device=dev)
                self.prefetch.stream = None
            self.text_cus = 0
            return
        total = device_cus(dev)
        text_cus = min(max(8, text_cus // 8 * 8), total - 8)       # whole CUs of every XCD on both sides
        torch.cuda.synchronize(dev)
        self.text_stream = partition_stream(dev, 0, text_cus)
        self.prefetch.stream = partition_stream(dev, text_cus, total - text_cus)
        self.text_cus = text_cus

    @property
    def prefetch_split(self) -> tuple:
        """(stop_block, cu_cap) of TRAINER.MVLPT.PREFETCH_SPLIT; (0, 0): the image tower in one piece."""
        return self.prefetch.split

    @prefetch_split.setter
    def prefetch_split(self, split) -> None:
        self.prefetch.split = split

    def split_active(self) -> bool:
        """The prefetch split applies: a split is set and nothing makes today's schedule the only one (the towers on one stream,
        visual prompts, a class-sharded text tower, a CU partition, a tower with fewer blocks than the split point)."""
        if getattr(self.engine, "resnet", False):
            return False      # a ResNet tower runs in one piece (no mvlpt_image_fwd_begin / _resume): the whole-tower prefetch stays
        layers = getattr(getattr(self.engine, "arch", None), "vision_layers", 0)
        # (a split point past the last full-width block is not a split of THIS tower: a default found on twelve blocks leaves a
        # two-block test tower in one piece; stop_block = layers - 1 is the old early-prefetch schedule, kept as the control)
        return (0 < self.prefetch_split[0] <= layers - 1 and self.overlap_towers and self.text_stream is not None
                and self._class_shard is None and self.text_cus == 0 and self.prompt_learner.vpt_embeddings is None)

    def has_prefetched(self, image) -> bool:
        return self.prefetch.get(image) is not None

    def prefetch_image_features(self, image, stop_block=None, cu_cap=None) -> bool:
        """Software pipelining across steps: with no visual prompts the image tower is a pure function of the image
        (frozen weights, trainers/mvlpt.py:855-858), so the features of the NEXT batch are computed on a third HIP stream
        beside the current step's text tower (forward, backward: small launches that cannot fill the chip), head and
        optimizer.  `forward(image)` picks the result up when it is called with the same tensor.  Successive prefetches
        queue up on that one stream (they share the tower workspace).

        Prefetch split: with `stop_block` > 0 (and `split_active`) only the first blocks are enqueued, capped at `cu_cap` compute
        units; a second call for the same tensor enqueues the rest (ImagePrefetch.start).  False: this model prefetches nothing."""
        if self.prompt_learner.vpt_embeddings is not None or self.text_stream is None:
            return False
        split = bool(stop_block) and self.split_active()
        self.prefetch.start(image, int(stop_block) if split else 0, int(cu_cap or 0))
        return True

    def drop_prefetch(self) -> None:
        """Forget prefetched image forwards that nobody will pick up (the loop left the loader early)."""
        self.prefetch.drop()

    def prompt_learner_visual_prompts(self):
        """(vpt, vpt_deep) as the image tower takes them: forward_mvlpt_proj, then vpt_proj (no dropout)."""
        return self.projected_prompts()[1:]

    def forward(self, image, task=None):
        coop_emb, vpt_emb, vpt_emb_deep = self.projected_prompts(batch=image.shape[0])
        lo = hi = None
        if self.multi_task_label_pertask:
            t = task.cpu().long() if torch.is_tensor(task) else torch.as_tensor(task).long()
            lo = self.class_index_pertask_start[t].to(torch.int32).to(image.device)
            hi = self.class_index_pertask_end[t].to(torch.int32).to(image.device)
        return _PromptedClipFn.apply(self, image, lo, hi, coop_emb, vpt_emb, vpt_emb_deep, torch.is_grad_enabled(),
                                     getattr(self.prompt_learner, "ctx_deep", None))

    def cross_entropy(self, logits, label):
        """HIP replacement for ``F.cross_entropy(output, label)`` (trainers/mvlpt.py:931)."""
        return _CrossEntropyFn.apply(self, logits, label)
