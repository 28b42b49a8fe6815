"""MVLPT's CoCoOp route on the HIP engine (-m gpu): the ranged glue kernels, the ranged head, the ranged text tower against the
class-specific-context tower (partial ranges and every range full), the model against the REAL reference's fixtures
(tools/make_mvlpt_cocoop_golden.py) at the project's criterion (max|d| <= 1e-3 max|ref|), ranged against dense,
chunking with the recompute-in-backward path, and the trainer."""
import numpy as np
import pytest
import torch

from tests.golden_util import load_npz, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-3
FOLD = {"off": (0, 4096), "forced": (2, 1)}          # set_ln_fold(mode, min_rows)
CASES = ["tiny_mvlpt_cocoop", "tiny_mvlpt_cocoop_mask", "tiny_mvlpt_cocoop_mask_soft", "tiny_mvlpt_cocoop_vpt",
         "tiny_mvlpt_cocoop_ctxinit", "tiny_mvlpt_cocoop_cut", "full_vitb16_mvlpt_cocoop_mask"]
MASK_CASES = ["tiny_mvlpt_cocoop_mask", "tiny_mvlpt_cocoop_mask_soft", "tiny_mvlpt_cocoop_vpt", "full_vitb16_mvlpt_cocoop_mask"]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _seqs(lo, hi):
    """(group, class) of every sequence of the ranges, in the tower's order."""
    return [(g, c) for g, (a, b) in enumerate(zip(lo, hi)) for c in range(a, b)]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("position", ["end", "middle"])
def test_ranged_assembly_bit_exact(position):
    from mvlpt_amd.engine import op_assemble_prompts_ranged
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(5)
    C, L, n, d = 7, 40, 5, 192
    lo, hi = [2, 4, 3, 0, 0], [5, 4, 4, 7, 2]                      # a middle range, an empty one, one class, the full range, a head
    G = len(lo)
    layout = build_prompt_layout([1, 2, 3, 1, 4, 2, 1], n, L, position)
    prefix, suffix = torch.randn(C, 1, d, generator=g), torch.randn(C, L - 1 - n, d, generator=g)
    ctx, pos = torch.randn(G, n, d, generator=g), torch.randn(L + 3, d, generator=g)
    got = op_assemble_prompts_ranged(prefix.to(DEV), suffix.to(DEV), ctx.to(DEV), layout.to(DEV), pos.to(DEV), lo, hi).cpu()
    fixed = torch.cat([prefix, suffix], dim=1)                                              # [C, L - n, d]
    table = torch.cat([fixed.unsqueeze(0).expand(G, -1, -1, -1), ctx.unsqueeze(1).expand(-1, C, -1, -1)], dim=2)   # [G, C, L, d]
    idx = torch.where(layout >= 0, layout, (L - n) + (-layout - 1)).long()                  # row of `table` per position
    dense = torch.gather(table, 2, idx.view(1, C, L, 1).expand(G, C, L, d)) + pos[:L]       # [G, C, L, d]
    seqs = _seqs(lo, hi)
    want = torch.stack([dense[gi, c] for gi, c in seqs])
    assert got.shape == (len(seqs), L, d) and len(seqs) == 3 + 0 + 1 + 7 + 2
    assert torch.equal(got, want)


def _ctx_pos(layout, n):
    C, L = layout.shape
    ctx_pos = torch.zeros(C, n, dtype=torch.int32)
    for c in range(C):
        for i in range(L):
            if layout[c, i] < 0:
                ctx_pos[c, -int(layout[c, i]) - 1] = i
    return ctx_pos


def test_ranged_ctx_grad_gather_deterministic_and_exact():
    from mvlpt_amd.engine import op_gather_ctx_grad, op_gather_ctx_grad_ranged
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(6)
    C, L, n, d = 37, 30, 6, 256
    lo, hi = [0, 5, 36, 9, 0, 20], [37, 7, 37, 9, 2, 37]            # full, 2 wide, 1 wide, empty, 2 wide, 17 wide (> 16 waves)
    G = len(lo)
    layout = build_prompt_layout([1 + c % 4 for c in range(C)], n, L, "middle")
    ctx_pos = _ctx_pos(layout, n)
    seqs = _seqs(lo, hi)
    dx = torch.randn(len(seqs), L, d, generator=g)
    a = op_gather_ctx_grad_ranged(dx.to(DEV), ctx_pos.to(DEV), lo, hi).cpu()
    b = op_gather_ctx_grad_ranged(dx.to(DEV), ctx_pos.to(DEV), lo, hi).cpu()
    assert torch.equal(a, b)
    want = torch.zeros(G, n, d, dtype=torch.float64)
    for s, (gi, c) in enumerate(seqs):
        want[gi] += dx[s].double()[ctx_pos[c].long()]
    assert float((a.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert torch.equal(a[3], torch.zeros(n, d)), "an empty range must give exact zeros"
    # every range full (CoCoOp's tower): group by group the bits of the generic-context gather over the group's C sequences
    G2 = 3
    dx2 = torch.randn(G2 * C, L, d, generator=g)
    full = op_gather_ctx_grad_ranged(dx2.to(DEV), ctx_pos.to(DEV), [0] * G2, [C] * G2).cpu()
    per_group = [op_gather_ctx_grad(dx2[k * C:(k + 1) * C].to(DEV), ctx_pos.to(DEV), False, None).cpu() for k in range(G2)]
    assert torch.equal(full, torch.stack(per_group))


@pytest.fixture(scope="module")
def tiny_clip():
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    return FrozenCLIP(make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True), device=DEV)


def test_ranged_head_fwd_bwd_against_float64(tiny_clip):
    eng = tiny_clip.engine
    e = tiny_clip.arch.embed_dim
    g = torch.Generator().manual_seed(7)
    C, scale = 9, 100.0
    lo, hi = [0, 3, 8, 4, 0], [9, 5, 9, 4, 2]
    G = len(lo)
    seqs = _seqs(lo, hi)
    S = len(seqs)
    img, txt = torch.randn(G, e, generator=g) * 3, torch.randn(S, e, generator=g) * 0.5
    dl = torch.randn(G, C, generator=g)
    logits = eng.logits_ranged_fwd(img.to(DEV), txt.to(DEV), scale, lo, hi, C)
    dimg, dtxt = eng.logits_ranged_bwd(dl.to(DEV), need_img=True, need_txt=True)
    img64, txt64 = img.double().requires_grad_(True), txt.double().requires_grad_(True)
    imn = img64 / img64.norm(dim=-1, keepdim=True)
    txn = txt64 / txt64.norm(dim=-1, keepdim=True)
    gi = torch.tensor([s[0] for s in seqs])
    ci = torch.tensor([s[1] for s in seqs])
    want = torch.zeros(G, C, dtype=torch.float64).index_put((gi, ci), scale * (imn[gi] * txn).sum(-1))
    want.backward(dl.double())
    inside = torch.zeros(G, C, dtype=torch.bool)
    inside[gi, ci] = True
    logits = logits.cpu()
    assert torch.equal(logits[~inside], torch.zeros(int((~inside).sum()))), "logits outside the ranges must be exactly 0"
    assert _rel(logits, want.detach()) <= 1e-5
    assert _rel(dtxt, txt64.grad) <= 1e-5
    assert _rel(dimg, img64.grad) <= 1e-5
    assert torch.equal(dimg[3].cpu(), torch.zeros(e)), "an image with an empty range gets no gradient"
    only_img, none_txt = eng.logits_ranged_bwd(dl.to(DEV), need_img=True, need_txt=False)
    assert none_txt is None and torch.equal(only_img, dimg)


# ------------------------------------------------------------------------------------------------ engine
def _tower_inputs(arch, G, g):
    from mvlpt_amd.model import build_prompt_layout
    C, L, n, dt = 5, 77, 4, arch.transformer_width
    layout = build_prompt_layout([1, 2, 2, 1, 3], n, L, "end").to(DEV)
    eot = torch.tensor([8, 9, 9, 8, 10], dtype=torch.int32, device=DEV)
    prefix = (torch.randn(C, 1, dt, generator=g) * 0.02).to(DEV)
    suffix = (torch.randn(C, L - 1 - n, dt, generator=g) * 0.02).to(DEV)
    ctx = (torch.randn(G, n, dt, generator=g) * 0.1).to(DEV)
    return C, L, n, dt, layout, eot, prefix, suffix, ctx


def test_ranged_text_tower_equals_csc_tower(tiny_clip):
    eng, arch = tiny_clip.engine, tiny_clip.arch
    g = torch.Generator().manual_seed(8)
    lo, hi = [1, 0, 3, 2, 0], [4, 5, 3, 3, 2]
    G = len(lo)
    C, L, n, dt, layout, eot, prefix, suffix, ctx = _tower_inputs(arch, G, g)
    seqs = _seqs(lo, hi)
    S = len(seqs)
    gi = torch.tensor([s[0] for s in seqs], device=DEV)
    ci = torch.tensor([s[1] for s in seqs], device=DEV)
    dfeat = torch.randn(S, arch.embed_dim, generator=g).to(DEV)
    fr = eng.text_fwd_ranged(prefix, suffix, ctx, layout, eot, lo, hi, save_for_bwd=True)
    dr = eng.text_bwd(dfeat)
    assert fr.shape == (S, arch.embed_dim) and dr.shape == (G, n, dt)
    # the same S sequences materialised for the class-specific-context tower: same sequence count, hence the same kernels
    fc = eng.text_fwd(prefix[ci], suffix[ci], ctx[gi], layout[ci], eot[ci], save_for_bwd=True)
    dc = eng.text_bwd(dfeat)
    torch.cuda.synchronize()
    assert torch.equal(fr, fc), "ranged features must be bit-identical to the materialised CSC tower"
    want = torch.zeros(G, n, dt, dtype=torch.float64, device=DEV).index_add_(0, gi, dc.double())
    assert float((dr.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert torch.equal(dr[2], torch.zeros_like(dr[2])), "empty range: zero context gradient"
    # no save: same features
    assert torch.equal(eng.text_fwd_ranged(prefix, suffix, ctx, layout, eot, lo, hi, save_for_bwd=False), fr)


def test_full_ranges_equal_csc_tower_and_float64_head(tiny_clip):
    """Every range full (CoCoOp's case) at the shapes of this file: the tower against the materialised class-specific-context tower
    (bit-equal features, context gradient within 1e-6 of the float64 sum over each image's classes), the head against float64 (1e-5);
    the bounds of tests/test_hip_cocoop.py."""
    eng, arch = tiny_clip.engine, tiny_clip.arch
    g = torch.Generator().manual_seed(9)
    G = 3
    C, L, n, dt, layout, eot, prefix, suffix, ctx = _tower_inputs(arch, G, g)
    e = arch.embed_dim
    dfeat = torch.randn(G * C, e, generator=g).to(DEV)
    img = torch.randn(G, e, generator=g).to(DEV)
    dl = torch.randn(G, C, generator=g).to(DEV)
    fr = eng.text_fwd_ranged(prefix, suffix, ctx, layout, eot, [0] * G, [C] * G, save_for_bwd=True)
    dr = eng.text_bwd(dfeat)
    lr = eng.logits_ranged_fwd(img, fr, 50.0, [0] * G, [C] * G, C)
    _, tr = eng.logits_ranged_bwd(dl)
    assert fr.shape == (G * C, e) and dr.shape == (G, n, dt) and lr.shape == (G, C) and tr.shape == (G * C, e)
    fc = eng.text_fwd(prefix.repeat(G, 1, 1), suffix.repeat(G, 1, 1), ctx.repeat_interleave(C, 0), layout.repeat(G, 1),
                      eot.repeat(G), save_for_bwd=True)
    dc = eng.text_bwd(dfeat)
    torch.cuda.synchronize()
    assert torch.equal(fr, fc), "full-range features must be bit-identical to the materialised CSC tower"
    want = dc.view(G, C, n, dt).double().sum(1)
    assert float((dr.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    img64, txt64 = img.double().cpu(), fr.double().cpu().requires_grad_(True)
    imn = img64 / img64.norm(dim=-1, keepdim=True)
    txn = (txt64 / txt64.norm(dim=-1, keepdim=True)).view(G, C, e)
    want = 50.0 * torch.einsum("ge,gce->gc", imn, txn)
    want.backward(dl.double().cpu())
    assert _rel(lr, want.detach()) <= 1e-5
    assert _rel(tr, txt64.grad) <= 1e-5


def test_ranged_calls_refuse_bad_ranges(tiny_clip):
    eng, arch = tiny_clip.engine, tiny_clip.arch
    g = torch.Generator().manual_seed(10)
    C, L, n, dt, layout, eot, prefix, suffix, ctx = _tower_inputs(arch, 2, g)
    for lo, hi in ([0, 0], [C + 1, C]), ([3, 0], [2, C]), ([-1, 0], [2, 2]), ([1, 2], [1, 2]), ([0], [C]):
        with pytest.raises(ValueError):
            eng.text_fwd_ranged(prefix, suffix, ctx, layout, eot, lo, hi)
    with pytest.raises(ValueError):
        eng.text_fwd_ranged(prefix, suffix, ctx, layout, eot, torch.tensor([0, 0], device=DEV), torch.tensor([C, C], device=DEV))


# ------------------------------------------------------------------------------------------------ model vs reference
def _case_clip(name, cache={}):
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    key = "tiny" if name.startswith("tiny") else "ViT-B/16"
    if key not in cache:
        sd = make_state_dict(ARCHS[key], 1 if key == "tiny" else 2, include_token_embedding=True)
        cache[key] = (FrozenCLIP(sd, device=DEV), sd)
    return cache[key]


def build_model(name, case=None):
    """(model, image, label (normalised when soft), task, case) on the GPU with the fixture's parameters and buffers."""
    from mvlpt_amd.model import PretokenizedPrompts
    from mvlpt_amd.mvlpt_cocoop import CustomCLIP
    from tests.test_mvlpt_cocoop_host import case_dm, mvlpt_cocoop_cfg
    case = case or load_npz(name)
    clip, sd = _case_clip(name)
    R = clip.arch.image_resolution
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist())
    model = CustomCLIP(mvlpt_cocoop_cfg(case, R), [str(c) for c in case["classnames"]], clip, dm=case_dm(case), pretokenized=pre)
    state = {k[len("param_"):]: t(v) for k, v in case.items() if k.startswith("param_")}
    if "image" in case:
        image = t(case["image"])
        state["token_prefix"], state["token_suffix"] = t(case["token_prefix"]), t(case["token_suffix"])
    else:
        gen = torch.Generator().manual_seed(int(case["image_seed"]))
        image = torch.randn(len(case["label"]), 3, R, R, generator=gen)
        emb = sd["token_embedding.weight"][t(case["tokenized_prompts"])]
        n = int(case["meta_n_ctx"])
        state["token_prefix"], state["token_suffix"] = emb[:, :1].contiguous(), emb[:, 1 + n:].contiguous()
    model.prompt_learner.load_state_dict(state, strict=True)
    assert np.array_equal(model.prompt_learner.layout.numpy(), case["layout"])
    model = model.to(DEV)
    label = t(case["label"])
    if label.dim() > 1:                                       # trainers/mvlpt.py:914-916
        label = label.float() / label.float().sum(dim=-1, keepdim=True)
    task = t(case["task"]) if "task" in case else None       # stays on the CPU, as in MVLPT.parse_batch_train
    return model, image.to(DEV), label.to(DEV), task, case


def run_model(model, image, label, task):
    pl = model.prompt_learner
    pl.train()
    pl.zero_grad(set_to_none=True)
    logits = model(image, task=task)
    loss = model.cross_entropy(logits, label)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in pl.named_parameters()}


def _margins(case, logits, loss, grads):
    m = {"logits": _rel(logits, t(case["out_logits"]))}
    m["loss"] = abs(float(loss) - float(case["out_loss"]))
    for k, g in grads.items():
        m["grad " + k] = _rel(g, t(case["grad_" + k]))
    return m


def _outside(case, logits):
    """the logits outside every image's task range"""
    lo, hi = t(case["task_start"])[t(case["task"])], t(case["task_end"])[t(case["task"])]
    idx = torch.arange(logits.shape[1]).unsqueeze(0)
    return logits.cpu()[~((idx >= lo.unsqueeze(1)) & (idx < hi.unsqueeze(1)))]


@pytest.mark.parametrize("trim", [False, True], ids=["full_len", "trim_eot"])
@pytest.mark.parametrize("fold", list(FOLD))
@pytest.mark.parametrize("name", CASES)
def test_model_matches_reference(name, fold, trim):
    model, image, label, task, case = build_model(name)
    model.trim_text_to_eot = trim
    model.engine.set_ln_fold(*FOLD[fold])
    try:
        logits, loss, grads = run_model(model, image, label, task)
    finally:
        model.engine.set_ln_fold(2, 4096)
    margins = _margins(case, logits, loss, grads)
    print(f"{name} fold={fold} trim={trim}: " + ", ".join(f"{k} {v:.2e}" for k, v in margins.items()))
    want = {"cocoop_ctx", "meta_net.linear1.weight", "meta_net.linear1.bias", "meta_net.linear2.weight", "meta_net.linear2.bias"}
    if int(case["meta_vpt_n_ctx"]):
        want |= {"vpt_embeddings", "vpt_embeddings_deep"}
    assert set(grads) == want
    bad = {k: v for k, v in margins.items() if not v <= TOL}
    assert not bad, f"{name} fold={fold} trim={trim}: outside 1e-3 of the reference: {bad}"
    if task is not None:
        out = _outside(case, logits)
        assert out.numel() > 0 and bool((out == 0.0).all()), "logits outside the task range must be exactly 0"


@pytest.mark.parametrize("name", MASK_CASES)
def test_ranged_and_dense_agree_with_reference(name):
    model, image, label, task, case = build_model(name)
    L = model.prompt_learner.layout.shape[1]
    res = {}
    for ranged in (True, False):
        model.ranged_text = ranged
        logits, loss, grads = run_model(model, image, label, task)
        m = _margins(case, logits, loss, grads)
        print(f"{name} ranged={ranged}: sequences {model.last_sequences}, " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
        bad = {k: v for k, v in m.items() if not v <= TOL}
        assert not bad, f"{name} ranged={ranged}: outside 1e-3 of the reference: {bad}"
        assert bool((_outside(case, logits) == 0.0).all())
        res[ranged] = (model.last_sequences, model.engine.text_workspace_bytes(model.last_sequences, L, True))
    B, C = case["out_logits"].shape
    assert res[False][0] == B * C
    assert res[True][0] == int((case["task_end"][case["task"]] - case["task_start"][case["task"]]).sum()) < res[False][0]
    assert res[True][1] < res[False][1]


# ------------------------------------------------------------------------------------------------ chunking
@pytest.mark.parametrize("vpt", [False, True], ids=["plain", "vpt"])
def test_chunked_step_matches_one_chunk_and_is_deterministic(vpt):
    """>= 3 chunks (the forward saves nothing, the backward re-runs each chunk's forward) against one chunk, with an image whose
    task has no classes (an empty range) inside a chunk."""
    name = "tiny_mvlpt_cocoop_vpt" if vpt else "tiny_mvlpt_cocoop_mask"
    case = dict(load_npz(name))
    g = torch.Generator().manual_seed(9)
    counts = [2, 1, 3, 0]                                      # task 3 owns no class: an empty range
    task = np.array([2, 3, 0, 1, 2, 0, 3, 2])
    B = len(task)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    case["image"] = torch.randn(B, 3, 32, 32, generator=g).numpy()
    case["task"], case["task_counts"] = task, np.array(counts)
    case["label"] = np.array([starts[k] + (i % max(counts[k], 1)) if counts[k] else 0 for i, k in enumerate(task)], dtype=np.int64)
    model, image, label, task_t, _ = build_model(name, case)
    logits1, loss1, g1 = run_model(model, image, label, task_t)
    assert model.last_chunks == 1 and not model.last_recompute and model.last_sequences == 3 + 0 + 2 + 1 + 3 + 2 + 0 + 3
    L = model.prompt_learner.layout.shape[1]
    model.max_text_workspace_bytes = model.engine.text_workspace_bytes(5, L, True)
    logits_a, loss_a, ga = run_model(model, image, label, task_t)
    assert model.last_chunks >= 3 and model.last_recompute
    logits_b, loss_b, gb = run_model(model, image, label, task_t)
    assert torch.equal(loss_a, loss_b) and torch.equal(logits_a, logits_b)
    assert all(torch.equal(ga[k], gb[k]) for k in ga), "two identical chunked runs must be bit-identical"
    assert abs(float(loss_a) - float(loss1)) <= 1e-4 * max(1.0, abs(float(loss1)))
    assert _rel(logits_a, logits1) <= 1e-4
    assert bool((logits_a[1] == 0.0).all()) and bool((logits_a[6] == 0.0).all())
    for k in g1:
        assert _rel(ga[k], g1[k]) <= 1e-4, k


def test_stale_forward_is_refused():
    model, image, label, task, _ = build_model("tiny_mvlpt_cocoop_vpt")
    model.prompt_learner.train()
    loss = model.cross_entropy(model(image, task=task), label)
    model(image, task=task)
    with pytest.raises(RuntimeError, match="stale forward"):
        loss.backward()


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(tmp_path, vpt=0):
    from mvlpt_amd.class_prompts import MultitaskBook
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.TRAINER.MVLPT.COCOOP.N_CTX = 4
    cfg.TRAINER.MVLPT.VPT.N_CTX = vpt
    cfg.DATASET.MULTITASK = cfg.DATASET.MULTITASK_LABEL_PERTASK = True
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 6
    cfg.OPTIM.LR, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.MAX_EPOCH = 0.05, 0, 10
    cfg.OUTPUT_DIR = str(tmp_path)
    book = MultitaskBook([("pets", ["dog", "cat"]), ("things", ["grand piano", "airplane", "bus"]), ("sea", ["sea horse"])])
    dm = SyntheticDataManager(cfg, num_classes=book.num_classes, steps_per_epoch=1, seed=3, book=book)
    return MVLPT(cfg, dm=dm), dm


@pytest.mark.parametrize("vpt", [0, 2], ids=["plain", "vpt"])
def test_trainer_steps_match_plain_sgd_and_lower_loss(tmp_path, vpt):
    from mvlpt_amd.mvlpt_cocoop import CustomCLIP
    tr, dm = _trainer(tmp_path, vpt)
    assert type(tr.model) is CustomCLIP
    tr.num_batches, tr.batch_idx = 100, 0
    pl = tr.model.prompt_learner
    p0 = {k: v.detach().clone() for k, v in pl.named_parameters()}
    batch = dm.train_loader_x[0]
    losses = [float(tr.forward_backward(batch)["loss"]) for _ in range(3)]
    assert tr.model.last_sequences == sum(dm.task_class_counts[k] for k in batch["domain"].tolist()) < 6 * dm.num_classes
    p_tr = {k: v.detach().clone() for k, v in pl.named_parameters()}
    assert losses[2] < losses[0], losses
    with torch.no_grad():
        for k, v in pl.named_parameters():
            v.copy_(p0[k])
    params = [p for p in pl.parameters()]
    for p in params:
        p.grad = None
    o = tr.cfg.OPTIM
    sgd = torch.optim.SGD(params, lr=o.LR, momentum=o.MOMENTUM, weight_decay=o.WEIGHT_DECAY, dampening=o.SGD_DAMPNING,
                          nesterov=o.SGD_NESTEROV)
    image, label, task = batch["img"].to(DEV), batch["label"].to(DEV), batch["domain"]
    ref_losses = []
    for _ in range(3):
        sgd.zero_grad()
        loss = tr.model.cross_entropy(tr.model(image, task=task), label)
        loss.backward()
        sgd.step()
        ref_losses.append(float(loss))
    assert np.allclose(losses, ref_losses, rtol=1e-6, atol=1e-7), (losses, ref_losses)
    for k, v in pl.named_parameters():
        assert _rel(v.detach(), p_tr[k]) <= 1e-6, k


def test_trainer_test_returns_per_task_results(tmp_path):
    tr, dm = _trainer(tmp_path)
    res = tr.test()
    assert 0.0 <= res <= 100.0
    seen = {dm._task_names[k] for k in dm.test_loader[0]["domain"].tolist()}
    assert set(tr.last_task_results) == seen and all(0.0 <= v <= 100.0 for v in tr.last_task_results.values())


def test_load_model_roundtrips_checkpoint(tmp_path):
    import os
    tr, _ = _trainer(tmp_path, vpt=2)
    pl = tr.model.prompt_learner
    sd = {k: v.detach().cpu().clone() for k, v in pl.state_dict().items()}
    want = {k: v + 0.25 for k, v in sd.items()}               # a checkpoint with other values everywhere, buffers included
    d = os.path.join(str(tmp_path), "ckpt", "prompt_learner")
    os.makedirs(d)
    torch.save({"state_dict": want, "epoch": 3, "optimizer": None, "scheduler": None}, os.path.join(d, "model-best.pth.tar"))
    tr.load_model(os.path.join(str(tmp_path), "ckpt"))
    got = {k: v.detach().cpu() for k, v in pl.state_dict().items()}
    import json
    from tests.golden_util import GOLDEN
    assert list(got) == list(json.load(open(os.path.join(GOLDEN, "ref_mvlpt_cocoop_prompt_learner.json")))["state_dict_vpt"])
    for k in got:
        ref = sd[k] if k in ("token_prefix", "token_suffix") else want[k]      # the class buffers stay this model's own
        assert torch.equal(got[k], ref), k
