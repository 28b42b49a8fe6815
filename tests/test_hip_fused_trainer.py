"""OPTIM.FUSED at trainer level: the one-launch HIP optimizer step (mvlpt_amd.optim) behind the trainers' unchanged surface —
the reference's train fixture, checkpoints that cross between the fused and the torch.optim route in both directions, the
evaluation text cache, a prompt tensor without a gradient, a step with a non-finite loss, and build_optimizer's new names.

One-step bound (tests/test_hip_optim.py): |a - b| <= k * 2^-24 * T per element, k = 8 for SGD and 32 for Adam / AdamW, T the sum of
the absolute values of the terms that enter the element (tests/optim_ref.py)."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def make_trainer(tmp_path, fused, method="upt", name="sgd", classes=6, tasks=None, steps=4, B=8, cls=None):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    from mvlpt_amd.weights import ARCHS, make_state_dict
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = B
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.LR, cfg.OPTIM.WARMUP_EPOCH = 3, 0.05, 0
    cfg.OPTIM.NAME, cfg.OPTIM.FUSED = name, fused
    cfg.TRAIN.PRINT_FREQ = 1000
    if method in ("coop", "upt"):
        cfg.TRAINER.MVLPT.COOP.N_CTX = 4
    if method in ("vpt", "upt"):
        cfg.TRAINER.MVLPT.VPT.N_CTX = 2
    cfg.TRAINER.MVLPT.PROJECT_DIM = 64
    if tasks:
        cfg.DATASET.MULTITASK = True
        cfg.DATASET.MULTITASK_LABEL_PERTASK = True
    dm = SyntheticDataManager(cfg, classes, steps, task_class_counts=tasks, device="cuda", seed=3)
    torch.manual_seed(0)                                         # the prompt learner's initial values: the same for every trainer
    return (cls or MVLPT)(cfg, dm=dm, clip_state_dict=make_state_dict(ARCHS["tiny"], seed=9))


def train_steps(tr, k):
    tr.set_model_mode("train")
    tr.num_batches = 10 ** 6
    losses = []
    for tr.batch_idx in range(k):
        losses.append(float(tr.forward_backward(tr.train_loader_x[tr.batch_idx % len(tr.train_loader_x)])["loss"]))
    return losses


def views_intact(tr):
    fp, fg = tr._flat_params["prompt_learner"], tr._flat_grads["prompt_learner"]
    return fp.intact() and fg.intact() and all(isinstance(p, torch.nn.Parameter) and p.is_leaf for p in fp.params)


# ------------------------------------------------------------------------------------------------ the reference's train fixture
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_three_reference_train_steps_with_the_fused_optimizer(tmp_path, prec):
    """tests/golden/tiny_train_steps.npz through run_epoch with OPTIM.FUSED on; the tolerances of the torch-SGD test on the same
    fixture (tests/test_hip_trainer.py): losses 1e-3, every parameter's update within 2e-3 of its maximum."""
    from mvlpt_amd.model import PretokenizedPrompts
    from mvlpt_amd.optim import FusedSGD
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    from tests.golden_util import load_npz, t, tiny_state_dict
    from tests.train_step_util import check_against_fixture, fixture_cfg, run_three_steps
    z = load_npz("tiny_train_steps")
    cfg = fixture_cfg(z)
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.TRAINER.MVLPT.PREC = prec
    cfg.OPTIM.FUSED = True
    dm = SyntheticDataManager(cfg, 5, 1, device="cuda", seed=3)
    dm.pretokenized = PretokenizedPrompts(t(z["tokenized_prompts"]), z["name_lens"].tolist())
    tr = MVLPT(cfg, dm=dm, clip_state_dict=tiny_state_dict())
    assert isinstance(tr.optim, FusedSGD) and views_intact(tr)
    keys = list(tr.model.prompt_learner.state_dict())
    losses, lrs, params = run_three_steps(tr, z, "cuda")
    check_against_fixture(z, losses, lrs, params, loss_tol=1e-3, delta_tol=2e-3)
    assert views_intact(tr) and list(tr.model.prompt_learner.state_dict()) == keys     # load_state_dict copied in place
    assert tr.optim.skipped() == 0


# ------------------------------------------------------------------------------------------------ checkpoints cross the routes
def _one_more_step_agrees(a, b, kind, hyper, k):
    """Both optimizers hold the same values and state; one step from identical gradients; parameters and state within the
    one-step bound."""
    gen = torch.Generator().manual_seed(11)
    pa, pb = a.param_groups[0]["params"], b.param_groups[0]["params"]
    before = []
    for x, y in zip(pa, pb):
        assert torch.equal(x.detach(), y.detach())
        g = torch.randn(x.shape, generator=gen).cuda() * 0.1
        x.grad, y.grad = g.clone(), g.clone()
        sa, sb = a.state.get(x, {}), b.state.get(y, {})
        for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            assert (key in sa) == (key in sb), key
            if key in sa:
                assert torch.equal(sa[key], sb[key]), key
        if "step" in sa:
            assert float(sa["step"]) == float(sb["step"])
        before.append((x.detach().clone(), g, {k_: (v.detach().clone() if torch.is_tensor(v) else v) for k_, v in sa.items()}))
    a.step()
    b.step()
    torch.cuda.synchronize()
    f64 = lambda t_: t_.detach().cpu().numpy().astype(np.float64).ravel()
    h = hyper
    for (p0, g, st), x, y in zip(before, pa, pb):
        sa, sb = a.state[x], b.state[y]
        if kind == R.SGD:
            first = "momentum_buffer" not in st
            buf = np.zeros(p0.numel()) if first else f64(st["momentum_buffer"])
            Tp, Tb = R.sgd_terms(f64(p0), f64(g), buf, first, h["lr"], h["weight_decay"], h["momentum"], h["dampening"], h["nesterov"])
            pairs = [(x, y, Tp), (sa["momentum_buffer"], sb["momentum_buffer"], Tb)]
        else:
            t = int(float(st["step"])) + 1 if st else 1
            assert float(sa["step"]) == float(sb["step"]) == t
            m, v = (f64(st["exp_avg"]), f64(st["exp_avg_sq"])) if st else (np.zeros(p0.numel()), np.zeros(p0.numel()))
            Tp, Tm, Tv = R.adam_terms(f64(p0), f64(g), m, v, t, h["lr"], h["weight_decay"], h["beta1"], h["beta2"], h["eps"], kind == R.ADAMW)
            pairs = [(x, y, Tp), (sa["exp_avg"], sb["exp_avg"], Tm), (sa["exp_avg_sq"], sb["exp_avg_sq"], Tv)]
        for u_, v_, T in pairs:
            ratio = float((np.abs(f64(u_) - f64(v_)) / (U * T + 1e-300)).max())
            assert ratio <= k, f"the routes differ by {ratio:.2f} * 2^-24 * T after one step (bound {k})"
        assert not torch.equal(x.detach(), p0)


def _sgd_hyper(cfg):
    o = cfg.OPTIM
    return dict(lr=o.LR, weight_decay=o.WEIGHT_DECAY, momentum=o.MOMENTUM, dampening=o.SGD_DAMPNING, nesterov=o.SGD_NESTEROV)


@pytest.mark.parametrize("writer_fused", [True, False], ids=["fused-to-torch", "torch-to-fused"])
def test_checkpoint_resumes_on_the_other_route(tmp_path, writer_fused):
    """2 steps on one route, save_model (Dassl's dict), load into a trainer on the other route, one more step on both."""
    w = make_trainer(tmp_path / "w", writer_fused)
    train_steps(w, 2)
    w.save_model(1, str(tmp_path))
    ck = torch.load(os.path.join(str(tmp_path), "prompt_learner", "model.pth.tar-2"), map_location="cpu")
    assert set(ck) == {"state_dict", "epoch", "optimizer", "scheduler", "val_result"}
    assert set(ck["optimizer"]) == {"state", "param_groups"}
    assert all(set(s) == {"momentum_buffer"} for s in ck["optimizer"]["state"].values()) and ck["optimizer"]["state"]
    r = make_trainer(tmp_path / "r", not writer_fused)
    r.load_model(str(tmp_path), epoch=2)
    r.optim.load_state_dict(ck["optimizer"])
    r.sched.load_state_dict(ck["scheduler"])
    for t_ in (w, r):
        if t_.cfg.OPTIM.FUSED:
            assert views_intact(t_)
            fused = t_.optim
            for i, p in enumerate(fused._params):               # the state tensors still ARE the views of the flat state buffer
                if p in fused.state:
                    assert fused.state[p]["momentum_buffer"].data_ptr() == fused._view1[i].data_ptr()
    _one_more_step_agrees(w.optim, r.optim, R.SGD, _sgd_hyper(w.cfg), 8)


@pytest.mark.parametrize("name,kind", [("adam", R.ADAM), ("adamw", R.ADAMW)])
@pytest.mark.parametrize("writer_fused", [True, False], ids=["fused-to-torch", "torch-to-fused"])
def test_adam_state_dict_crosses_the_routes(name, kind, writer_fused):
    """FusedAdam(W).state_dict() <-> torch.optim.Adam(W).load_state_dict at optimizer level: 2 steps (one parameter sits the second
    out, so the step counts differ), state across, one more step on both."""
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.distributed import FlatGradients, FlatParameters
    from mvlpt_amd.trainer import build_optimizer
    shapes = [(5, 3), (1025,), (7,)]
    wd = 5e-4 if kind == R.ADAM else 1e-2

    def make(fused):
        g = torch.Generator().manual_seed(2)
        mod = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in shapes])
        cfg = get_cfg_default()
        cfg.OPTIM.NAME, cfg.OPTIM.LR, cfg.OPTIM.WEIGHT_DECAY, cfg.OPTIM.FUSED = name, 0.01, wd, fused
        flat = (FlatParameters(mod.parameters()), FlatGradients(mod.parameters())) if fused else None
        return mod, build_optimizer(mod, cfg.OPTIM, flat)

    wmod, w = make(writer_fused)
    rmod, r = make(not writer_fused)
    gen = torch.Generator().manual_seed(4)
    for step in range(2):
        for i, p in enumerate(wmod):
            p.grad = None if (step == 1 and i == 2) else torch.randn(p.shape, generator=gen).cuda()
        w.step()
    sd = copy.deepcopy(w.state_dict())          # as a checkpoint holds it (load_state_dict aliases the `step` tensors of a live dict)
    assert [float(sd["state"][i]["step"]) for i in range(3)] == [2.0, 2.0, 1.0]
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    with torch.no_grad():
        for p, q in zip(rmod, wmod):
            p.copy_(q)
    r.load_state_dict(sd)
    hyper = dict(lr=0.01, weight_decay=wd, beta1=0.9, beta2=0.999, eps=1e-8)
    _one_more_step_agrees(w, r, kind, hyper, 32)
    fused = w if writer_fused else r
    assert fused._fp.intact() and fused._steps == [3, 3, 2]
    for i, p in enumerate(fused._params):
        assert fused.state[p]["exp_avg"].data_ptr() == fused._view1[i].data_ptr()
        assert fused.state[p]["exp_avg_sq"].data_ptr() == fused._view2[i].data_ptr()


# ------------------------------------------------------------------------------------------------ what the raw kernel must not break
def test_eval_text_cache_is_refreshed_after_a_fused_step(tmp_path):
    """tests/test_hip_trainer.py::test_eval_accuracy_and_text_cache with the key on: the cache is keyed on the parameters' versions,
    which the kernel does not touch by itself."""
    tr = make_trainer(tmp_path, True, "coop", classes=6, tasks=[2, 1, 3])
    acc = tr.test()
    assert 0.0 <= acc <= 100.0
    model = tr.model
    assert model.text_cache.eval_key is not None
    ver0, txt0 = model.text_cache.eval_key, model.text_cache.eval_features.clone()
    tr.test()
    assert model.text_cache.eval_key == ver0
    tr.set_model_mode("train")
    tr.num_batches, tr.batch_idx = 10, 0
    tr.forward_backward(tr.train_loader_x[0])
    tr.test()
    assert model.text_cache.eval_key != ver0
    assert not torch.equal(model.text_cache.eval_features, txt0)       # ... and the text features are those of the NEW prompts


def test_a_prompt_tensor_without_a_gradient_is_not_touched(tmp_path):
    from mvlpt_amd.trainer import MVLPT

    class WithUnusedPrompt(MVLPT):
        def build_optim(self, name, module):
            module.unused_prompt = torch.nn.Parameter(torch.randn(3, 5, device=self.device))      # no forward reads it
            return super().build_optim(name, module)

    tr = make_trainer(tmp_path, True, "upt", cls=WithUnusedPrompt)
    p = tr.model.prompt_learner.unused_prompt
    keep = p.detach().clone()
    others = {n: q.detach().clone() for n, q in tr.model.prompt_learner.named_parameters() if q is not p}
    train_steps(tr, 3)
    assert p.grad is None and torch.equal(p.detach(), keep) and p not in tr.optim.state
    for n, q in tr.model.prompt_learner.named_parameters():
        if q is not p:
            assert q.grad is not None and not torch.equal(q.detach(), others[n]), n
    assert views_intact(tr)


def test_a_step_with_a_non_finite_loss_is_not_applied(tmp_path):
    """The loss handed to the optimizer is replaced by NaN for one step (the engine is not touched): prompts and momentum stay
    bit-identical, and run_epoch raises at its next PRINT_FREQ check."""
    tr = make_trainer(tmp_path, True, "upt")
    train_steps(tr, 1)
    real_step = tr.optim.step
    poisoned = []

    def nan_step(loss_dev=None):
        assert loss_dev is not None and loss_dev.is_cuda                 # forward_backward hands the step's loss over
        poisoned.append(float(loss_dev))
        return real_step(loss_dev=torch.full_like(loss_dev, float("nan")))

    pl = tr.model.prompt_learner
    snap = lambda: ({n: p.detach().clone() for n, p in pl.named_parameters()}, tr.optim._state1.clone())
    p0, m0 = snap()
    tr.optim.step = nan_step
    train_steps(tr, 1)
    tr.optim.step = real_step
    p1, m1 = snap()
    assert len(poisoned) == 1 and np.isfinite(poisoned[0])
    assert all(torch.equal(p0[n], p1[n]) for n in p0) and torch.equal(m0, m1)
    tr.cfg.TRAIN.PRINT_FREQ = 2
    tr.epoch = 0
    with pytest.raises(FloatingPointError):
        tr.run_epoch()
    assert tr.batch_idx == 1                                             # ... at the first check, not later
    tr.batch_hook = lambda i: i < 2
    tr.run_epoch()                                                       # reported once: the next check passes


# ------------------------------------------------------------------------------------------------ build_optimizer
@pytest.mark.parametrize("fused", [False, True])
def test_adamw_trains_on_both_routes(tmp_path, fused):
    from mvlpt_amd.optim import FusedAdamW
    tr = make_trainer(tmp_path, fused, "coop", name="adamw")
    assert isinstance(tr.optim, torch.optim.AdamW) and isinstance(tr.optim, FusedAdamW) == fused
    tr.optim.param_groups[0]["lr"] = 0.002
    losses = train_steps(tr, 12)
    assert sum(losses[-4:]) < sum(losses[:4]), losses


def test_cocoop_trainer_on_the_fused_route(tmp_path):
    from mvlpt_amd.cocoop import CoCoOp
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.optim import FusedSGD
    from mvlpt_amd.trainer import SyntheticDataManager
    out = []
    for fused in (False, True):
        cfg = get_cfg_default()
        cfg.MODEL.BACKBONE.NAME, cfg.INPUT.SIZE, cfg.TRAINER.NAME = "tiny", (32, 32), "CoCoOp"
        cfg.TRAINER.COCOOP.N_CTX = 4
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
        cfg.OPTIM.LR, cfg.OPTIM.WARMUP_EPOCH, cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.FUSED = 0.05, 0, 10, fused
        cfg.OUTPUT_DIR = str(tmp_path)
        dm = SyntheticDataManager(cfg, num_classes=6, steps_per_epoch=1, seed=3)
        torch.manual_seed(0)
        tr = CoCoOp(cfg, dm=dm)
        assert isinstance(tr.optim, FusedSGD) == fused
        tr.num_batches, tr.batch_idx = 100, 0
        losses = [float(tr.forward_backward(dm.train_loader_x[0])["loss"]) for _ in range(3)]
        out.append((losses, [p.detach().clone() for p in tr.model.prompt_learner.parameters()]))
    assert out[1][0][2] < out[1][0][0] and np.allclose(out[0][0], out[1][0], rtol=1e-5, atol=1e-6), out
    for p, q in zip(out[0][1], out[1][1]):
        assert float((p - q).abs().max()) <= 1e-5 * float(p.abs().max()) + 1e-7


def test_what_the_fused_route_refuses():
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.distributed import FlatGradients, FlatParameters
    from mvlpt_amd.optim import FusedAdam, FusedSGD
    from mvlpt_amd.trainer import build_optimizer
    mod = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(4, 4).cuda()), torch.nn.Parameter(torch.randn(3).cuda())])
    flat = (FlatParameters(mod.parameters()), FlatGradients(mod.parameters()))
    cfg = get_cfg_default()
    cfg.OPTIM.FUSED = True
    for name in ("amsgrad", "rmsprop", "radam"):
        cfg.OPTIM.NAME = name
        with pytest.raises(ValueError):
            build_optimizer(mod, cfg.OPTIM, flat)
    cfg.OPTIM.NAME = "adam"
    cfg.OPTIM.AMSGRAD = True
    with pytest.raises(ValueError):
        build_optimizer(mod, cfg.OPTIM, flat)
    cfg.OPTIM.AMSGRAD, cfg.OPTIM.STAGED_LR = False, True
    with pytest.raises(ValueError):
        build_optimizer(mod, cfg.OPTIM, flat)
    cfg.OPTIM.STAGED_LR = False
    with pytest.raises(ValueError):
        build_optimizer(mod, cfg.OPTIM)                                  # the fused route needs the flat buffers
    with pytest.raises(ValueError):
        FusedAdam(flat[0], flat[1], amsgrad=True)
    opt = FusedSGD(flat[0], flat[1], lr=0.1)
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2).cuda())]})      # one param group
    cfg.OPTIM.FUSED, cfg.OPTIM.NAME = False, "adamw"
    assert type(build_optimizer(mod, cfg.OPTIM)) is torch.optim.AdamW
