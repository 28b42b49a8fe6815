"""Nearest vocabulary words of a learned prompt, on the device.  Takes the positional arguments of the reference's
scripts/interpret_prompt.py (`fpath topk`) and prints its lines:

    python tools/interpret_prompt.py output/.../prompt_learner/model.pth.tar-50 5 [--backbone ViT-B/16] [--weights clip_state_dict.pt]

A generic context (`ctx` [n_ctx, width]) prints exactly what the reference script prints, so the two outputs can be diffed;
class-specific contexts (`ctx` [n_cls, n_ctx, width], which the reference refuses) and `cocoop_ctx` print the same lines under a
`name:` line each.  Only the token table is needed, not the towers: --weights names a file that holds CLIP's state dict (saved with
torch.save, bare or under a "state_dict" key) and its `token_embedding.weight` is used; without it the table is the seeded one
FrozenCLIP falls back to for --backbone, and the first line says so: the words then only show that the pipeline runs.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TABLE_KEY = "token_embedding.weight"


def load_table(backbone: str, weights):
    """(token table fp32 [vocab, width] on the host, whether it is the seeded stand-in)."""
    from mvlpt_amd.weights import ARCHS, _randn
    if weights is None:
        if backbone not in ARCHS:
            raise SystemExit(f"unknown --backbone {backbone!r}; known: {', '.join(ARCHS)}")
        arch = ARCHS[backbone]
        return _randn(TABLE_KEY, 0, (arch.vocab_size, arch.transformer_width), 0.02), True      # FrozenCLIP._token_table, token_seed 0
    if not os.path.isfile(weights):
        raise SystemExit(f"--weights {weights}: no such file")
    blob = torch.load(weights, map_location="cpu")
    tensors = blob.get("state_dict", blob) if isinstance(blob, dict) else {}
    if TABLE_KEY not in tensors:
        raise SystemExit(f"--weights {weights}: expected a state dict with {TABLE_KEY}")
    return tensors[TABLE_KEY].detach().float(), False


class TokenTable:
    """What mvlpt_amd.interpret needs of a FrozenCLIP, for a table alone: the handle-free kernel entry against a device copy."""

    def __init__(self, table: torch.Tensor):
        from mvlpt_amd.model import default_tokenizer
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = table.to(self.device).contiguous()
        self.tokenizer = default_tokenizer()
        self.engine = self

    def nearest_tokens(self, q, k):
        from mvlpt_amd.engine import op_nearest_rows
        idx, dist = op_nearest_rows(q, self.table, k)
        return idx.long(), dist


def main(argv=None) -> int:
    from mvlpt_amd.interpret import CONTEXT_KEYS, format_lines, interpret_state_dict
    ap = argparse.ArgumentParser(description="nearest vocabulary words of the context vectors in a prompt_learner checkpoint")
    ap.add_argument("fpath", help="checkpoint of the prompt learner (a Dassl model.pth.tar-N file)")
    ap.add_argument("topk", type=int, help="how many nearest words to list per context vector")
    ap.add_argument("--backbone", default="ViT-B/16", help="architecture of the seeded table when --weights is not given")
    ap.add_argument("--weights", default=None, help="file with CLIP's state dict; its token_embedding.weight is the table")
    args = ap.parse_args(argv)
    if not os.path.isfile(args.fpath):
        raise SystemExit(f"{args.fpath}: no such checkpoint")
    table, seeded = load_table(args.backbone, args.weights)
    contexts = torch.load(args.fpath, map_location="cpu")
    contexts = contexts.get("state_dict", contexts)
    if seeded:
        print(f"No CLIP weights given (--weights): seeded token table of {args.backbone} (FrozenCLIP's fallback); the words are not CLIP's")
    print(f"Return the top-{args.topk} matched words")
    print(f"Size of token embedding: {table.shape}")
    for key in CONTEXT_KEYS:
        if key in contexts:
            print(f"Size of context{'' if key == 'ctx' else ' (' + key + ')'}: {contexts[key].shape}")
    result = interpret_state_dict(contexts, TokenTable(table), args.topk)
    generic_only = list(result) == ["ctx"] and not isinstance(result["ctx"], dict)
    for line in format_lines(result["ctx"] if generic_only else result):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
