"""CPU restatement of test-time prompt tuning for tests/test_hip_tpt.py: the towers are oracle/clip_oracle.py's own functions (fp32),
the head is tests/tpt_ref.py (float64), the optimizer torch.optim.AdamW.  One image at a time, as the published method runs."""
import math

import torch

from oracle import clip_oracle as O
from tests import tpt_ref as R

G, V, K, N_CTX = 3, 8, 2, 4
NAMES = ["dog", "grand piano", "sea horse", "airplane", "great white shark", "cat", "red fox"]
N_CLASSES = 6                 # 5 to 7 classes
H_BAR = 1e-3                  # the project's bar, relative to max(1, .)
# The frozen CLIP of the path test is the synthetic test-size one with CLIP's trained logit scale, exp(logit_scale) = 100 (the
# synthetic default, 14.3, leaves every view's prediction near uniform: entropy gaps of 1e-3).  VIEW_SEED is the first seed of
# make_views for which gaps_ok holds after one step (searched on the CPU with this module; nothing else went into the choice).
LOGIT_SCALE_EXP = 100.0
VIEW_SEED = 9


def state_dict(arch, seed=1):
    from mvlpt_amd.weights import make_state_dict
    sd = make_state_dict(arch, seed, include_token_embedding=True)
    sd["logit_scale"] = torch.tensor(math.log(LOGIT_SCALE_EXP))
    return sd


def make_views(arch, seed=VIEW_SEED):
    """[G, V, 3, R, R]: independent random images (the widest spread of confidences a random tower gives)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(G, V, 3, arch.image_resolution, arch.image_resolution, generator=g)


def tune_ref(sd, arch, tables, ctx0, views, k, steps, lr, weight_decay=0.01):
    """tables: dict(prefix, suffix, layout, eot) of the prompt learner (CPU).  Returns per image lists over the steps of loss, H, sel,
    dctx, then the tuned contexts [G, n_ctx, dt] and the final logits [G, C]."""
    scale = float(sd["logit_scale"].exp())
    out = {"loss": [], "H": [], "sel": [], "dctx": [], "ctx": [], "logits": []}
    for g in range(views.shape[0]):
        feats, _ = O.image_encoder_fwd(sd, views[g], None, None, heads=arch.vision_heads, need_bwd=False)
        ctx = torch.nn.Parameter(ctx0.clone())
        opt = torch.optim.AdamW([ctx], lr=lr, weight_decay=weight_decay)
        rec = {"loss": [], "H": [], "sel": [], "dctx": []}
        for _ in range(steps):
            prompts = O.assemble_prompts(ctx.detach(), tables["prefix"], tables["suffix"], tables["layout"])
            txt, tctx = O.text_encoder_fwd(sd, prompts, tables["eot"].long(), heads=arch.transformer_heads, need_bwd=True)
            loss, H, sel, dtxt, _ = R.tpt_ref(feats.unsqueeze(0), txt, scale, k)
            dx = O.text_encoder_bwd(sd, dtxt.float(), tctx)
            dctx = O.scatter_prompt_grad(dx, tables["layout"], tuple(ctx.shape))
            rec["loss"].append(loss[0]); rec["H"].append(H[0]); rec["sel"].append(sel[0]); rec["dctx"].append(dctx)
            ctx.grad = dctx.clone()
            opt.step()
        prompts = O.assemble_prompts(ctx.detach(), tables["prefix"], tables["suffix"], tables["layout"])
        txt, _ = O.text_encoder_fwd(sd, prompts, tables["eot"].long(), heads=arch.transformer_heads, need_bwd=False)
        logits, _ = O.logits_fwd(feats[:1], txt, scale, None)
        for n in rec:
            out[n].append(rec[n])
        out["ctx"].append(ctx.detach().clone())
        out["logits"].append(logits[0])
    out["ctx"], out["logits"] = torch.stack(out["ctx"]), torch.stack(out["logits"])
    return out


def gaps_ok(ref, k):
    """Every image, every step: the float64 gap between the k-th and (k+1)-th smallest entropy is at least 100 x the bar on H."""
    worst = float("inf")
    for per_image in ref["H"]:
        for H in per_image:
            gap = float(R.boundary_gap(H.unsqueeze(0), k)[0]) / max(1.0, float(H.abs().max()))
            worst = min(worst, gap)
    return worst >= 100 * H_BAR, worst
