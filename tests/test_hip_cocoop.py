"""CoCoOp on the HIP engine (-m gpu): the ranged glue kernels, text tower and head with every range full (one context block per image
against every class), the tower against the existing CSC tower, the model
against the REAL reference's fixtures (tools/make_cocoop_golden.py) at the project's criterion (max|d| <= 1e-3 max|ref|),
chunking, and the trainer's step."""
import numpy as np
import pytest
import torch

from tests.golden_util import load_npz, t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-3
COCOOP_CASES = ["tiny_cocoop", "tiny_cocoop_ctxinit", "full_vitb16_cocoop"]
FOLD = {"off": (0, 4096), "forced": (2, 1)}          # set_ln_fold(mode, min_rows); the library default is (2, 4096)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# ------------------------------------------------------------------------------------------------ kernels
def _grouped_assembly_bit_exact(G, C, L, n, d, name_lens, position):
    from mvlpt_amd.engine import op_assemble_prompts_ranged
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(5)
    layout = build_prompt_layout(name_lens, n, L, position)
    prefix, suffix = torch.randn(C, 1, d, generator=g), torch.randn(C, L - 1 - n, d, generator=g)
    ctx, pos = torch.randn(G, n, d, generator=g), torch.randn(L + 3, d, generator=g)
    got = op_assemble_prompts_ranged(prefix.to(DEV), suffix.to(DEV), ctx.to(DEV), layout.to(DEV), pos.to(DEV), [0] * G, [C] * G).cpu()
    fixed = torch.cat([prefix, suffix], dim=1)                                              # [C, L - n, d]
    table = torch.cat([fixed.unsqueeze(0).expand(G, -1, -1, -1), ctx.unsqueeze(1).expand(-1, C, -1, -1)], dim=2)   # [G, C, L, d]
    idx = torch.where(layout >= 0, layout, (L - n) + (-layout - 1)).long()                  # row of `table` per position
    want = torch.gather(table, 2, idx.view(1, C, L, 1).expand(G, C, L, d)) + pos[:L]
    assert torch.equal(got, want.reshape(G * C, L, d))


@pytest.mark.parametrize("position", ["end", "middle"])
def test_grouped_assembly_bit_exact(position):
    _grouped_assembly_bit_exact(3, 7, 40, 5, 192, [1, 2, 3, 1, 4, 2, 1], position)


def test_grouped_assembly_bit_exact_capped_grid():
    """(300, 77, 512), the capped-grid shape of tests/test_hip_glue.py::test_assemble_prompts_bit_exact, with two groups: 5.9 M float4
    items against the 8192 x 256 threads of the capped grid, so every thread takes a second and a third stride (CoCoOp's real shapes
    always do), and the later strides belong to the second group."""
    C = 300
    _grouped_assembly_bit_exact(2, C, 77, 5, 512, [1 + c % 4 for c in range(C)], "middle")


def test_grouped_ctx_grad_gather_deterministic_and_exact():
    from mvlpt_amd.engine import op_gather_ctx_grad_ranged
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(6)
    G, C, L, n, d = 4, 37, 30, 6, 256
    layout = build_prompt_layout([1 + c % 4 for c in range(C)], n, L, "middle")
    ctx_pos = torch.zeros(C, n, dtype=torch.int32)
    for c in range(C):
        for i in range(L):
            if layout[c, i] < 0:
                ctx_pos[c, -int(layout[c, i]) - 1] = i
    dx = torch.randn(G * C, L, d, generator=g)
    a = op_gather_ctx_grad_ranged(dx.to(DEV), ctx_pos.to(DEV), [0] * G, [C] * G).cpu()
    b = op_gather_ctx_grad_ranged(dx.to(DEV), ctx_pos.to(DEV), [0] * G, [C] * G).cpu()
    assert torch.equal(a, b)
    rows = dx.double().view(G, C, L, d)[:, torch.arange(C).view(C, 1), ctx_pos.long()]      # [G, C, n, d]
    want = rows.sum(1)
    assert float((a.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.fixture(scope="module")
def tiny_clip():
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    return FrozenCLIP(make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True), device=DEV)


def test_grouped_head_fwd_bwd_against_float64(tiny_clip):
    eng = tiny_clip.engine
    e = tiny_clip.arch.embed_dim
    g = torch.Generator().manual_seed(7)
    G, C, scale = 5, 9, 100.0
    img, txt = torch.randn(G, e, generator=g) * 3, torch.randn(G * C, e, generator=g) * 0.5
    dl = torch.randn(G, C, generator=g)
    logits = eng.logits_ranged_fwd(img.to(DEV), txt.to(DEV), scale, [0] * G, [C] * G, C)
    dimg, dtxt = eng.logits_ranged_bwd(dl.to(DEV), need_img=False, need_txt=True)
    assert dimg is None
    img64, txt64 = img.double(), txt.double().requires_grad_(True)
    imn = img64 / img64.norm(dim=-1, keepdim=True)
    txn = (txt64 / txt64.norm(dim=-1, keepdim=True)).view(G, C, e)
    want = scale * torch.einsum("ge,gce->gc", imn, txn)
    want.backward(dl.double())
    assert _rel(logits, want.detach()) <= 1e-5
    assert _rel(dtxt, txt64.grad) <= 1e-5


# ------------------------------------------------------------------------------------------------ engine
def test_grouped_text_tower_equals_csc_tower(tiny_clip):
    """The ranged entry with every range full against the plain kernels.  (1, 17): a single group with more classes than the gather has waves; (2, 16):
    exactly one class per wave."""
    from mvlpt_amd.model import build_prompt_layout
    eng, arch = tiny_clip.engine, tiny_clip.arch
    g = torch.Generator().manual_seed(8)
    L, n, dt = 77, 4, arch.transformer_width
    for G, C in ((3, 5), (1, 17), (2, 16)):
        name_lens = ([1, 2, 2, 1, 3] * 4)[:C]
        layout = build_prompt_layout(name_lens, n, L, "end").to(DEV)
        eot = torch.tensor([7 + k for k in name_lens], dtype=torch.int32, device=DEV)
        prefix = (torch.randn(C, 1, dt, generator=g) * 0.02).to(DEV)
        suffix = (torch.randn(C, L - 1 - n, dt, generator=g) * 0.02).to(DEV)
        ctx = (torch.randn(G, n, dt, generator=g) * 0.1).to(DEV)
        dfeat = torch.randn(G * C, arch.embed_dim, generator=g).to(DEV)
        fg = eng.text_fwd_ranged(prefix, suffix, ctx, layout, eot, [0] * G, [C] * G, save_for_bwd=True)
        dg = eng.text_bwd(dfeat)
        assert fg.shape == (G * C, arch.embed_dim) and dg.shape == (G, n, dt)
        fc = eng.text_fwd(prefix.repeat(G, 1, 1), suffix.repeat(G, 1, 1), ctx.repeat_interleave(C, 0), layout.repeat(G, 1),
                          eot.repeat(G), save_for_bwd=True)
        dc = eng.text_bwd(dfeat)
        torch.cuda.synchronize()
        assert torch.equal(fg, fc), f"G={G} C={C}: full-range features must be bit-identical to the materialised CSC tower"
        want = dc.view(G, C, n, dt).double().sum(1)
        assert float((dg.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()), f"G={G} C={C}"
        per_image = eng.text_workspace_bytes(C, L, True)
        assert per_image > 0 and (G == 1 or eng.text_workspace_bytes(G * C, L, True) > per_image)


def test_head_backward_follows_only_its_own_forward(tiny_clip):
    """logits_bwd and logits_ranged_bwd each run after the forward of their own name and raise after the other's."""
    eng = tiny_clip.engine
    e = tiny_clip.arch.embed_dim
    g = torch.Generator().manual_seed(11)
    G, C = 2, 3
    img, txt_c = torch.randn(G, e, generator=g).to(DEV), torch.randn(C, e, generator=g).to(DEV)
    txt_gc = torch.randn(G * C, e, generator=g).to(DEV)
    dl = torch.randn(G, C, generator=g).to(DEV)
    forwards = {
        "plain": lambda: eng.logits_fwd(img, txt_c, 10.0),
        "ranged": lambda: eng.logits_ranged_fwd(img, txt_gc, 10.0, [0] * G, [C] * G, C),
    }
    backwards = {
        "plain": lambda: eng.logits_bwd(dl),
        "ranged": lambda: eng.logits_ranged_bwd(dl),
    }
    for f, fwd in forwards.items():
        for b, bwd in backwards.items():
            assert fwd().shape == (G, C)
            if b == f:
                bwd()
            else:
                with pytest.raises(RuntimeError, match=r"call logits\w*_fwd first"):
                    bwd()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ model vs reference
def _case_clip(name, cache={}):
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    key = "tiny" if name.startswith("tiny") else "ViT-B/16"
    if key not in cache:
        sd = make_state_dict(ARCHS[key], 1 if key == "tiny" else 2, include_token_embedding=True)
        cache[key] = (FrozenCLIP(sd, device=DEV), sd)
    return cache[key]


def build_cocoop(name, case=None):
    """(model, image, label, case) on the GPU with the fixture's parameters and buffers."""
    from mvlpt_amd.cocoop import CustomCLIP
    from mvlpt_amd.model import PretokenizedPrompts
    from tests.test_cocoop_host import cocoop_cfg
    case = case or load_npz(name)
    clip, sd = _case_clip(name)
    R = clip.arch.image_resolution
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist())
    model = CustomCLIP(cocoop_cfg(case, R), [str(c) for c in case["classnames"]], clip, pretokenized=pre)
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
    return model, image.to(DEV), t(case["label"]).to(DEV), case


def run_cocoop(model, image, label):
    pl = model.prompt_learner
    pl.eval()
    logits = model(image)
    pl.train()
    pl.zero_grad(set_to_none=True)
    loss = model(image, label)
    loss.backward()
    torch.cuda.synchronize()
    return logits, loss.detach(), {k: p.grad.detach().clone() for k, p in pl.named_parameters()}


@pytest.mark.parametrize("trim", [False, True], ids=["full_len", "trim_eot"])
@pytest.mark.parametrize("fold", list(FOLD))
@pytest.mark.parametrize("name", COCOOP_CASES)
def test_model_matches_reference(name, fold, trim):
    model, image, label, case = build_cocoop(name)
    model.trim_text_to_eot = trim
    model.engine.set_ln_fold(*FOLD[fold])
    try:
        logits, loss, grads = run_cocoop(model, image, label)
    finally:
        model.engine.set_ln_fold(2, 4096)
    margins = {"logits": _rel(logits, t(case["out_logits"]))}
    margins["loss"] = abs(float(loss) - float(case["out_loss"])) / max(1.0, abs(float(case["out_loss"])))
    for k, g in grads.items():
        margins["grad " + k] = _rel(g, t(case["grad_" + k]))
    print(f"{name} fold={fold} trim={trim}: " + ", ".join(f"{k} {v:.2e}" for k, v in margins.items()))
    assert len(grads) == 5
    bad = {k: v for k, v in margins.items() if not v <= TOL}
    assert not bad, f"{name} fold={fold} trim={trim}: outside 1e-3 of the reference: {bad}"


# ------------------------------------------------------------------------------------------------ chunking
def test_chunked_step_matches_one_chunk_and_is_deterministic():
    case = load_npz("tiny_cocoop")
    g = torch.Generator().manual_seed(9)
    B = 7
    case = dict(case)
    case["image"] = torch.randn(B, 3, 32, 32, generator=g).numpy()
    case["label"] = torch.randint(0, 5, (B,), generator=g).numpy()
    model, image, label, _ = build_cocoop("tiny_cocoop", case)
    _, loss1, g1 = run_cocoop(model, image, label)
    assert model.last_chunks == 1
    L = model.prompt_learner.layout.shape[1]
    model.max_text_workspace_bytes = model.engine.text_workspace_bytes(2 * model.prompt_learner.n_cls, L, True)
    logits_a, loss_a, ga = run_cocoop(model, image, label)
    assert model.last_chunks >= 3
    logits_b, loss_b, gb = run_cocoop(model, image, label)
    assert torch.equal(loss_a, loss_b) and torch.equal(logits_a, logits_b)
    assert all(torch.equal(ga[k], gb[k]) for k in ga), "two identical chunked runs must be bit-identical"
    assert abs(float(loss_a) - float(loss1)) <= 1e-4 * max(1.0, abs(float(loss1)))
    for k in g1:
        assert _rel(ga[k], g1[k]) <= 1e-4, k


# ------------------------------------------------------------------------------------------------ trainer
def _trainer(tmp_path):
    from mvlpt_amd.cocoop import CoCoOp
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import SyntheticDataManager
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.TRAINER.NAME = "CoCoOp"
    cfg.TRAINER.COCOOP.N_CTX = 4
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    cfg.OPTIM.LR, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.MAX_EPOCH = 0.05, 0, 10
    cfg.OUTPUT_DIR = str(tmp_path)
    dm = SyntheticDataManager(cfg, num_classes=6, steps_per_epoch=1, seed=3)
    return CoCoOp(cfg, dm=dm), dm


def test_trainer_step_matches_plain_sgd_and_lowers_loss(tmp_path):
    tr, dm = _trainer(tmp_path)
    tr.num_batches, tr.batch_idx = 100, 0
    pl = tr.model.prompt_learner
    p0 = {k: v.detach().clone() for k, v in pl.named_parameters()}
    batch = dm.train_loader_x[0]
    losses = [float(tr.forward_backward(batch)["loss"]) for _ in range(3)]
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
    image, label = batch["img"].to(DEV), batch["label"].to(DEV)
    ref_losses = []
    for _ in range(3):
        sgd.zero_grad()
        loss = tr.model(image, label)
        loss.backward()
        sgd.step()
        ref_losses.append(float(loss))
    assert np.allclose(losses, ref_losses, rtol=1e-6, atol=1e-7), (losses, ref_losses)
    for k, v in pl.named_parameters():
        assert _rel(v.detach(), p_tr[k]) <= 1e-6, k


def test_load_model_roundtrips_reference_checkpoint(tmp_path):
    import os
    tr, _ = _trainer(tmp_path)
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
    assert list(got) == list(json.load(open(os.path.join(GOLDEN, "ref_cocoop_prompt_learner.json")))["state_dict"])
    for k in got:
        ref = sd[k] if k in ("token_prefix", "token_suffix") else want[k]      # the class buffers stay this model's own
        assert torch.equal(got[k], ref), k
