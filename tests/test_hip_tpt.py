"""Test-time prompt tuning on the HIP engine at path level (-m gpu): mvlpt_amd.tpt.CustomCLIP.tune and the TPT trainer against the CPU
restatement of tests/tpt_path_ref.py (oracle towers, float64 head, torch AdamW) at the project's bar, 1e-3 relative to max.

The selection is compared exactly.  That is fair only where the restatement's own entropies leave no near-tie: the float64 gap at the
selection boundary must be at least 100 x the bar on H for every image, which is asserted on the CPU side before the device is looked
at (tests/tpt_path_ref.py says how the inputs were chosen).  The tuned contexts get the same treatment: AdamW's first step is
lr * g / (|g| + eps), the SIGN of the gradient, so an element whose reference gradient lies within the bar of zero has no decided
step; those elements (under 1 % here, asserted) are held to one step's length instead, every other element to the bar."""
import os

import pytest
import torch

from tests import tpt_path_ref as P
from tests import tpt_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-3
LR = 5e-3


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def make_cfg(arch, steps=1, fused=False):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (arch.image_resolution,) * 2
    cfg.TRAINER.TPT.N_VIEWS, cfg.TRAINER.TPT.SELECTION_P, cfg.TRAINER.TPT.STEPS, cfg.TRAINER.TPT.LR = P.V, P.K / P.V, steps, LR
    cfg.OPTIM.FUSED = fused
    return cfg


@pytest.fixture(scope="module")
def setup():
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.tpt import CustomCLIP
    from mvlpt_amd.weights import ARCHS
    arch = ARCHS["tiny"]
    sd = P.state_dict(arch)
    clip = FrozenCLIP(sd, device=DEV)
    torch.manual_seed(0)
    model = CustomCLIP(make_cfg(arch), P.NAMES[:P.N_CLASSES], clip).to(DEV)
    assert (model.n_views, model.k, model.steps) == (P.V, P.K, 1)
    views = P.make_views(arch)
    pl = model.prompt_learner
    tables = dict(prefix=pl.token_prefix.cpu(), suffix=pl.token_suffix.cpu(), layout=pl.layout.cpu(), eot=pl.eot.cpu())
    ref = P.tune_ref(sd, arch, tables, pl.ctx.detach().cpu(), views, P.K, 1, LR)      # once, shared, never modified
    return arch, sd, clip, model, views, ref


def test_tune_against_the_cpu_restatement(setup):
    arch, sd, clip, model, views, ref = setup
    ok, worst = P.gaps_ok(ref, P.K)                            # the CPU side alone
    assert ok, worst
    ref_dctx = torch.stack([r[0] for r in ref["dctx"]])
    ref_loss = torch.stack([r[0] for r in ref["loss"]])
    ref_sel = torch.stack([r[0] for r in ref["sel"]])
    ref_H = torch.stack([r[0] for r in ref["H"]])
    decided = ref_dctx.abs() >= TOL * ref_dctx.abs().amax(dim=(1, 2), keepdim=True)
    assert float((~decided).float().mean()) <= 0.01
    ctx0 = model.prompt_learner.ctx.detach().clone()
    logits = model.tune(views.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(model.prompt_learner.ctx.detach(), ctx0)                         # ctx0 is never modified
    assert logits.shape == (P.G, P.N_CLASSES) and model.last_chunks == 1
    assert all(torch.is_tensor(t) and t.is_cuda for t in (model.last_loss, model.last_selected, model.last_entropy))
    figs = {"loss": _rel(model.last_loss, ref_loss), "H": R.rel_max1(model.last_entropy, ref_H),
            "dctx": max(_rel(model.last_dctx[g], ref_dctx[g]) for g in range(P.G)),
            "logits": _rel(logits, ref["logits"])}
    got_ctx, want_ctx = model.last_ctx.cpu(), ref["ctx"]
    err = (got_ctx.double() - want_ctx.double()).abs()
    figs["ctx"] = float(err[decided].max()) / float(want_ctx.abs().max())
    figs["ctx_undecided_abs"] = float(err[~decided].max()) if bool((~decided).any()) else 0.0
    print(" ".join(f"{n} {v:.3e}" for n, v in figs.items()), "gap", worst)
    assert torch.equal(model.last_selected.cpu().long(), ref_sel), (model.last_selected, ref_sel)
    for n in ("loss", "H", "dctx", "logits", "ctx"):
        assert figs[n] <= TOL, (n, figs[n])
    assert figs["ctx_undecided_abs"] <= 2 * LR * 1.01                                    # one step this way instead of that way
    assert float((got_ctx - ctx0.cpu()).abs().max()) > 0.5 * LR                         # the contexts did move


def _hand_driven(model, views, steps):
    """`steps` steps of tune driven by hand: tune_step + the same optimizer, then the final logits through the engine."""
    from mvlpt_amd.model import _text_inputs
    eng, pl = model.engine, model.prompt_learner
    G, V = views.shape[:2]
    feats = eng.image_fwd(views.reshape(G * V, *views.shape[2:]), None, None, save_for_bwd=False).view(G, V, -1)
    ctx = pl.ctx.detach().unsqueeze(0).expand(G, -1, -1).clone()
    holder, optim = model._optimizer(ctx)
    for _ in range(steps):
        _, _, _, dctx = model.tune_step(feats, holder.ctx.data)
        if holder.ctx.grad is None:
            holder.ctx.grad = dctx
        else:
            holder.ctx.grad.copy_(dctx)
        optim.step()
    suffix, layout = _text_inputs(model, pl, pl.coop_n_ctx)
    lo, hi = [0] * G, [pl.n_cls] * G
    txt = eng.text_fwd_ranged(pl.token_prefix, suffix, holder.ctx.data, layout, pl.eot, lo, hi, save_for_bwd=False)
    return eng.logits_ranged_fwd(feats[:, 0].contiguous(), txt, model.logit_scale_exp, lo, hi, pl.n_cls), holder.ctx.data.clone()


@pytest.mark.parametrize("fused", [False, True], ids=["torch_adamw", "fused_adamw"])
def test_two_steps_agree_with_two_hand_driven_steps(setup, fused):
    from mvlpt_amd.tpt import CustomCLIP
    arch, sd, clip, model, views, ref = setup
    torch.manual_seed(0)
    m2 = CustomCLIP(make_cfg(arch, steps=2, fused=fused), P.NAMES[:P.N_CLASSES], clip).to(DEV)
    with torch.no_grad():
        got = m2.tune(views.to(DEV))
        ctx2 = m2.last_ctx.clone()
        want, want_ctx = _hand_driven(m2, views.to(DEV), 2)
        one, _ = _hand_driven(m2, views.to(DEV), 1)
    assert torch.equal(got, want) and torch.equal(ctx2, want_ctx)
    assert not torch.equal(got, one)                                                    # the second step did something
    if fused:                                                                           # the one-launch AdamW agrees with torch's
        assert _rel(ctx2, _hand_driven(model_with(m2, steps=2, fused=False, arch=arch, clip=clip), views.to(DEV), 2)[1]) <= TOL


def model_with(like, steps, fused, arch, clip):
    from mvlpt_amd.tpt import CustomCLIP
    torch.manual_seed(0)
    return CustomCLIP(make_cfg(arch, steps=steps, fused=fused), P.NAMES[:P.N_CLASSES], clip).to(DEV)


def test_zero_steps_is_the_untuned_prompt(setup):
    arch, sd, clip, model, views, ref = setup
    m0 = model_with(model, 0, False, arch, clip)
    logits = m0.tune(views.to(DEV))
    pl = m0.prompt_learner
    txt = clip.engine.text_fwd(pl.token_prefix, pl.token_suffix, pl.ctx.detach(), pl.layout, pl.eot, save_for_bwd=False)
    feats = clip.engine.image_fwd(views[:, 0].to(DEV).contiguous(), None, None, save_for_bwd=False)
    want = clip.engine.logits_fwd(feats, txt, m0.logit_scale_exp)
    assert _rel(logits, want) <= 1e-5


def test_one_image_per_chunk_equals_the_unchunked_run(setup):
    arch, sd, clip, model, views, ref = setup
    whole = model.tune(views.to(DEV))
    loss, sel, dctx = model.last_loss.clone(), model.last_selected.clone(), model.last_dctx.clone()
    budget = model.max_text_workspace_bytes
    try:
        L = model.prompt_learner.layout.shape[1]
        model.max_text_workspace_bytes = clip.engine.text_workspace_bytes(P.N_CLASSES, L, True)      # one image's tower, no more
        assert model.images_per_chunk(P.G, L, True) == 1
        chunked = model.tune(views.to(DEV))
        assert model.last_chunks == P.G
        assert torch.equal(model.last_selected, sel)
        assert _rel(model.last_loss, loss) <= TOL and _rel(model.last_dctx, dctx) <= TOL and _rel(chunked, whole) <= TOL
    finally:
        model.max_text_workspace_bytes = budget


def test_a_coop_checkpoint_is_the_starting_point(setup, tmp_path):
    """A CoOp run's prompt_learner checkpoint (ctx [n_ctx, dt] plus the token buffers, which are dropped) loads through MVLPT.load_model
    into the TPT trainer, and `tune` starts from it."""
    from mvlpt_amd.tpt import TPT
    from mvlpt_amd.trainer import SyntheticDataManager
    arch, sd, clip, model, views, ref = setup
    cfg = make_cfg(arch, steps=0)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.TRAINER.MVLPT.COOP.N_CTX = 4                         # the CoOp run's own setting: random init, class in the middle
    dm = SyntheticDataManager(cfg, num_classes=P.N_CLASSES, steps_per_epoch=1, device=DEV)
    tr = TPT(cfg, dm=dm, clip_state_dict=sd)
    pl = tr.model.prompt_learner
    g = torch.Generator().manual_seed(4)
    ctx = torch.randn(4, arch.transformer_width, generator=g) * 0.02
    folder = tmp_path / "ckpt" / "prompt_learner"
    os.makedirs(folder)
    torch.save({"state_dict": {"ctx": ctx, "token_prefix": torch.zeros(1), "token_suffix": torch.zeros(1)}, "epoch": 7},
               folder / "model.pth.tar-7")
    before = pl.ctx.detach().clone()
    tr.load_model(str(tmp_path / "ckpt"), epoch=7)
    assert torch.equal(pl.ctx.detach().cpu(), ctx) and not torch.equal(before.cpu(), ctx)
    logits = tr.model.tune(views.to(DEV))                    # STEPS = 0: the loaded context, untouched
    assert torch.equal(tr.model.last_ctx.cpu(), ctx.unsqueeze(0).expand(P.G, -1, -1))
    txt = tr.model.engine.text_fwd(pl.token_prefix, pl.token_suffix, pl.ctx.detach(), pl.layout, pl.eot, save_for_bwd=False)
    feats = tr.model.engine.image_fwd(views[:, 0].to(DEV).contiguous(), None, None, save_for_bwd=False)
    assert _rel(logits, tr.model.engine.logits_fwd(feats, txt, tr.model.logit_scale_exp)) <= 1e-5
    with pytest.raises(RuntimeError, match="nothing to train"):
        tr.forward_backward(None)


def test_trainer_test_on_a_resident_set(tmp_path):
    """TPT.test() from DATASET.SOURCES: the test loader serves views of the resident test split, and the accuracy is the one computed
    from tune's logits on the same views."""
    from mvlpt_amd.tpt import TPT
    from mvlpt_amd.transforms import build_view_transform
    from mvlpt_amd.weights import ARCHS
    from tests.data_util import write_dataset
    arch = ARCHS["tiny"]
    root = str(tmp_path / "images")
    write_dataset(root)
    cfg = make_cfg(arch)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.DATASET.SOURCES = [["pets", "", root]]
    cfg.DATALOADER.TEST.BATCH_SIZE, cfg.DATALOADER.NUM_WORKERS = 4, 2
    tr = TPT(cfg, clip_state_dict=P.state_dict(arch))
    assert tr.dm.image_sets["test"] is not None and tr.test_loader.n_views == P.V and tr.dm.train_loader_x.n_views == 0
    acc = tr.test()
    # the same views by hand: one ViewTransform with the loader's seed over the resident set, batch after batch
    from mvlpt_amd.data import rank_seed
    vt = build_view_transform(cfg, tr.model.engine, P.V, generator=torch.Generator().manual_seed(rank_seed(cfg.SEED, 0)))
    n = len(tr.test_loader.dataset)
    labels = torch.tensor([it.label for it in tr.test_loader.dataset])
    hits = 0
    for b0 in range(0, n, 4):
        idx = list(range(b0, min(n, b0 + 4)))
        views = vt.from_resident(tr.dm.image_sets["test"], idx)
        assert views.shape == (len(idx), P.V, 3, arch.image_resolution, arch.image_resolution)
        hits += int((tr.model.tune(views).argmax(-1).cpu() == labels[idx]).sum())
    assert n == 9 and acc == pytest.approx(100.0 * hits / n, abs=1e-9)
    assert tr.last_eval is not None                          # the device metrics route (DeviceClassification) came with MVLPT.test
