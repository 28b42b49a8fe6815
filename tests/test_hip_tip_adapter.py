"""Tip-Adapter end to end on the test-size towers (-m gpu): the head built from synthetic images, Tip-Adapter-F lowering its training
loss, the first AdamW step against float64, the search against the float64 reference, the trainer's train() / test() and a
save / load round trip."""
import functools

import numpy as np
import pytest
import torch

from tests import tip_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_CLS, SHOTS, BATCH = 6, 4, 8
LR, EPS, WD = 1e-3, 1e-4, 0.01


@functools.lru_cache(maxsize=None)
def clip():
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    sd = make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True)
    return FrozenCLIP(sd, compute_dtype="fp16", device=DEV), sd


@functools.lru_cache(maxsize=None)
def few_shot():
    """(batches of (images, labels), all images, all labels): SHOTS images per class in a shuffled order, generated once."""
    c, _ = clip()
    g = torch.Generator().manual_seed(5)
    res = c.arch.image_resolution
    labels = torch.arange(N_CLS).repeat(SHOTS)[torch.randperm(N_CLS * SHOTS, generator=g)]
    images = torch.randn(N_CLS * SHOTS, 3, res, res, generator=g)
    images, labels = images.to(DEV), labels.to(DEV)
    batches = [(images[i:i + BATCH], labels[i:i + BATCH]) for i in range(0, len(labels), BATCH)]
    return batches, images, labels


def new_head(**kw):
    from mvlpt_amd.tip_adapter import TipAdapterHead
    c, _ = clip()
    g = torch.Generator().manual_seed(9)
    W = torch.randn(N_CLS, c.arch.embed_dim, generator=g)
    W = (W / W.norm(dim=-1, keepdim=True)).to(DEV)
    head = TipAdapterHead(c.engine, W, R.SCALE, **kw)
    return head.build_cache(c, lambda: few_shot()[0], augment_epochs=2)


def host(head, features):
    """The float32 arrays the device entries see, for the float64 reference."""
    F = head._unit(features).cpu().numpy()
    return {"F": F, "K": head.keys.cpu().numpy(), "key_ptr": head.key_ptr.cpu().numpy(), "key_cls": head.key_labels.numpy(),
            "W": head.text_features.cpu().numpy()}


def test_head_from_images():
    c, _ = clip()
    batches, images, labels = few_shot()
    head = new_head()
    assert head.keys.shape == (N_CLS * SHOTS, c.arch.embed_dim) and head.key_ptr.tolist() == [SHOTS * i for i in range(N_CLS + 1)]
    assert head.key_labels.tolist() == sorted(labels.tolist())
    feats = c.encode_image(images)
    # two identical passes: the mean of a unit row with itself, normalised again, is the row up to rounding
    order = np.argsort(labels.cpu().numpy(), kind="stable")
    assert torch.allclose(head.keys, head._unit(feats)[torch.from_numpy(order).to(DEV)], atol=1e-6)
    h = host(head, feats)
    z, dz = R.logits_bound(h["F"], h["K"], h["key_ptr"], h["W"], head.alpha, head.beta)
    got = head.logits(feats).cpu().numpy()
    assert np.all(np.abs(got - z) <= dz)
    assert torch.equal(head.predict(feats).cpu(), torch.from_numpy(got.argmax(1)))


def test_fit_lowers_the_training_loss():
    c, _ = clip()
    head = new_head()
    head.fit(c, lambda: few_shot()[0], epochs=3, lr=LR, eps=EPS)
    losses = [h[1] for h in head.history]
    print("Tip-Adapter-F training loss per epoch:", losses)
    assert len(losses) == 3 and losses[2] < losses[0]
    assert all(h[3] is None for h in head.history)


@pytest.mark.parametrize("fused", [False, True], ids=["torch", "fused"])
def test_first_step_is_a_float64_adamw_step(fused):
    """One batch, one epoch: the keys after the step against AdamW in float64 from the reference gradient.
    Tolerance, per element, with dg the dK bound of tests/tip_ref.py, g the reference gradient, u = 2^-24:
      the first step moves a key by lr h(g), h(g) = g / (|g| + eps) (bias-corrected moments of one gradient), h' = eps / (|g| + eps)^2
        decreasing in |g|, so a gradient within dg of g moves it by at most lr dg eps / (max(|g| - dg, 0) + eps)^2 more or less;
      the fp32 update itself: the two moments (3 roundings), their bias corrections and the square root (3), the sum with eps, the
        quotient, the product with the step size and the rounded constants 1 - beta1, 1 - beta2 (5): 12 u lr since |h| <= 1;
      the decay p (1 - lr wd) and the final sum: 4 u |p|;
      below |g| = 2^-63 the square of g leaves the normal fp32 range; there the exact and the computed update are both at most
        lr |g| / eps: 2 lr 2^-63 / eps."""
    c, _ = clip()
    batches, images, labels = few_shot()
    one = [(images[:BATCH], labels[:BATCH])]
    head = new_head(fused=fused)
    before = head.keys.clone()
    h = host(head, c.encode_image(one[0][0]))
    b = R.train_bounds(h["F"], one[0][1].cpu().numpy(), h["K"], h["key_ptr"], h["key_cls"], h["W"], head.alpha, head.beta)
    head.fit(c, lambda: one, epochs=1, lr=LR, eps=EPS)
    g, dg, p = b["ref"]["dK"], b["dK"], before.cpu().numpy().astype(np.float64)
    want = R.adamw_step(p, g, LR, eps=EPS, weight_decay=WD)
    tol = LR * dg * EPS / (np.maximum(np.abs(g) - dg, 0.0) + EPS) ** 2 + 12 * R.U * LR + 4 * R.U * np.abs(p) + 2 * LR * 2.0 ** -63 / EPS
    err = np.abs(head.keys.cpu().numpy().astype(np.float64) - want)
    print(f"first step ({'fused' if fused else 'torch'}): largest error / tolerance {float((err / tol).max()):.3f}, "
          f"largest move {float(np.abs(want - p).max()):.2e}")
    assert float(np.abs(want - p).max()) > 0.5 * LR          # the step moved the keys: the comparison means something
    assert np.all(err <= tol)
    assert abs(head.history[0][1] - b["ref"]["loss"]) <= b["loss"]


def test_search_against_the_reference():
    """The towers' features of random images all but coincide, so the search runs on the generator of tests/tip_ref.py instead: class
    prototypes, an unbalanced cache with an empty class, 200 noisy held-out rows.  tests/test_tip_ref.py asserts that the reference's
    winner leads every other grid point by more than twice the undecided rows, so the device must return it."""
    from mvlpt_amd.tip_adapter import TipAdapterHead, search_grid
    c, _ = clip()
    case = R.WINNER_CASE
    assert case[1] == c.arch.embed_dim
    data = R.make_case(*case, R.WINNER_SIGMA, R.WINNER_SEED)
    head = TipAdapterHead(c.engine, torch.from_numpy(data["W"]).to(DEV), R.SCALE)
    head.from_features(data["K"], data["key_cls"], len(case[2]))
    feats, labels = torch.from_numpy(data["F"]).to(DEV), torch.from_numpy(data["y"]).to(DEV)
    step = R.WINNER_STEP
    betas, alphas = search_grid((7.0, 3.0), step)
    h = host(head, feats)
    ref = R.search(h["F"], labels.cpu().numpy(), h["K"], h["key_ptr"], h["W"], np.float32(betas), np.float32(alphas))
    beta, alpha, acc, counts = head.search_hp(feats, labels, (7.0, 3.0), step)
    assert (ref["sure"] <= counts).all() and (counts <= ref["sure"] + ref["undecided"]).all()
    decided = ref["undecided"] == 0
    assert np.array_equal(counts[decided], ref["counts"][decided])
    wb, wa = R.winner(ref["counts"])
    others = ref["counts"].copy()
    others[wb, wa] = -1
    gap = ref["counts"][wb, wa] - others.max()
    print(f"search: counts {counts.min()} .. {counts.max()} of {len(labels)}, gap of the winner {gap}, undecided at most {ref['undecided'].max()}")
    assert gap > 2 * ref["undecided"].max()       # every count lies within `undecided` of the reference's: the winner cannot change
    assert (beta, alpha) == (betas[wb], alphas[wa])
    assert (head.beta, head.alpha) == (beta, alpha) and acc == pytest.approx(100.0 * counts.max() / len(labels))
    b, a = np.unravel_index(int(np.argmax(counts.ravel())), counts.shape)
    assert (beta, alpha) == (betas[b], alphas[a])          # the first maximum of its own counts


def _trainer(tmp_path, **tip):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.tip_adapter import TipAdapter
    from mvlpt_amd.trainer import SyntheticDataManager
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.TRAINER.NAME = "TipAdapter"
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = BATCH
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.TRAINER.TIP.AUGMENT_EPOCH = 2
    cfg.TRAINER.TIP.SEARCH_STEP = [7, 5]
    for k, v in tip.items():
        cfg.TRAINER.TIP[k] = v
    dm = SyntheticDataManager(cfg, num_classes=N_CLS, steps_per_epoch=3, seed=3)
    dm.classnames = ["dog", "cat", "sea_horse", "oak", "bus", "violin"]
    return TipAdapter(cfg, dm=dm, clip_state_dict=clip()[1])


@pytest.mark.parametrize("finetune", [False, True], ids=["tip", "tip-f"])
def test_trainer_end_to_end(tmp_path, finetune, capsys):
    tr = _trainer(tmp_path, FINETUNE=finetune, TRAIN_EPOCH=2)
    with pytest.raises(RuntimeError, match="cache is empty"):
        tr.model_inference(tr.dm.test_loader[0]["img"].to(DEV))
    result = tr.train()
    out = capsys.readouterr().out
    assert "the search runs on the TEST loader" in out and "Tip-Adapter search: beta" in out
    batch = tr.dm.test_loader[0]
    logits = tr.model_inference(batch["img"].to(DEV))
    assert logits.shape == (BATCH, N_CLS)
    want = 100.0 * float((logits.argmax(1).cpu() == batch["label"]).sum()) / BATCH
    assert result == pytest.approx(want) and tr.test() == pytest.approx(want)
    assert tr.head.keys.shape[0] == 3 * BATCH and len(tr.head.history) == (2 if finetune else 0)
    # a second trainer loads what the first one saved: the same logits, bit for bit
    tr2 = _trainer(tmp_path)
    tr2.load_model(str(tmp_path))
    assert (tr2.head.alpha, tr2.head.beta) == (tr.head.alpha, tr.head.beta)
    assert torch.equal(tr2.model_inference(batch["img"].to(DEV)), logits)
    tr2.load_model(str(tmp_path), epoch=2 if finetune else 1)
    assert torch.equal(tr2.model_inference(batch["img"].to(DEV)), logits)
    with pytest.raises(FileNotFoundError):
        tr2.load_model(str(tmp_path), epoch=99)


def test_trainer_from_image_files(tmp_path, capsys):
    """DATASET.SOURCES: the train loader reshuffles on every pass and drops its last partial batch, which is right for fit() and wrong
    for a cache.  The cache comes from the loader's ordered pass: all 18 images, AUGMENT_EPOCH passes with equal labels."""
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.tip_adapter import TipAdapter
    from tests.data_util import write_dataset
    root = str(tmp_path / "images")
    items = write_dataset(root)
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.TRAINER.NAME = "TipAdapter"
    cfg.DATASET.SOURCES = [["pets", "", root]]
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    cfg.DATALOADER.TEST.BATCH_SIZE = 4
    cfg.DATALOADER.NUM_WORKERS = 2
    cfg.OUTPUT_DIR = str(tmp_path / "out")
    cfg.TRAINER.TIP.AUGMENT_EPOCH = 3
    cfg.TRAINER.TIP.SEARCH_STEP = [7, 5]
    cfg.TRAINER.TIP.FINETUNE = True
    cfg.TRAINER.TIP.TRAIN_EPOCH = 2
    tr = TipAdapter(cfg, clip_state_dict=clip()[1])
    n = len(items["train"])
    assert n == 18 and len(tr.train_loader_x) == 4 and n % 4 != 0        # the shuffled loader would drop two images
    result = tr.train()
    out = capsys.readouterr().out
    assert "TEST loader" not in out                                    # there is a validation split: the search runs on it
    assert tr.head.keys.shape[0] == n and tr.head.key_labels.tolist() == sorted(lab for _, lab, _ in items["train"])
    assert tr.head.key_ptr.tolist() == [0, 6, 12, 18]
    assert len(tr.head.history) == 2 and all(h[3] is not None for h in tr.head.history)
    assert 0.0 <= result <= 100.0 and result == pytest.approx(tr.test())
