"""The fused optimizer step at kernel level (mvlpt_op_optim_step, csrc/optim.hip) against the float64 reference of
tests/optim_ref.py (pinned to torch.optim by tests/test_optim_ref.py).

Bound, per element: |kernel - reference| <= k * 2^-24 * T, the reference evaluated in float64 from the DEVICE's own fp32 inputs of
that step (errors do not compound across steps) and T the sum of the absolute values of the terms that enter the element
(optim_ref.sgd_terms / adam_terms).  k = 8 for SGD: p' is at most 7 fp32 roundings away (d; m * buf and the sum; d + m * buf; lr * upd
and the difference; 1 - dampening is formed in double on the host and rounded once), with or without FMA contraction.  k = 32 for
Adam / AdamW (the denominator adds a square root, two divisions and beta^t).  The kernel computes beta1^t and beta2^t ONCE per segment
in DOUBLE (exponentiation by squaring) and rounds lr / (1 - beta1^t) and sqrt(1 - beta2^t) to fp32 once each, as torch.optim does
with its Python floats: the power contributes no fp32 error, so nothing is added to the bound.  Indices are 64-bit throughout the
kernel; a buffer past 2^31 elements (8 GiB per buffer, four of them) is not exercised here.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CANARY = 64
MAIN_LENGTHS = [1, 3, 5, 1023, 1025, 4099, 2]          # n = 6158: not a multiple of 4, unaligned boundaries, one segment over 5 blocks
SGD_HYPERS = [
    dict(lr=0.05, weight_decay=5e-4, momentum=0.9, dampening=0.0, nesterov=False),
    dict(lr=0.05, weight_decay=5e-4, momentum=0.9, dampening=0.0, nesterov=True),
    dict(lr=0.05, weight_decay=0.0, momentum=0.9, dampening=0.1, nesterov=False),
    dict(lr=0.05, weight_decay=5e-4, momentum=0.0, dampening=0.0, nesterov=False),
]
ADAM_HYPERS = [(R.ADAM, dict(lr=0.01, weight_decay=5e-4, beta1=0.9, beta2=0.999, eps=1e-8)),
               (R.ADAM, dict(lr=0.01, weight_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8)),
               (R.ADAMW, dict(lr=0.01, weight_decay=1e-2, beta1=0.9, beta2=0.999, eps=1e-8))]


def f32(x):
    return float(np.float32(x))


def as_f32(hyper):
    """Hyper-parameters that fp32 holds exactly: the kernel's fp32 copies of lr / weight decay / momentum / beta2 / eps are then the
    values the float64 reference is evaluated with (the struct carries doubles, as torch.optim does)."""
    return {k: (v if isinstance(v, bool) else f32(v)) for k, v in hyper.items()}


class Buffers:
    """param / grad / state1 / state2 of n floats, each inside an allocation with 64-float canaries on both sides; the buffer starts
    256 bytes into its allocation."""

    def __init__(self, n, gen, dev="cuda"):
        self.n = n
        self.raw = {}
        for name in ("param", "grad", "s1", "s2"):
            self.raw[name] = torch.full((n + 2 * CANARY,), 12345.0 + len(self.raw), dtype=torch.float32, device=dev)
        self.param.copy_(torch.randn(n, generator=gen))
        self.s1.zero_()
        self.s2.zero_()
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)

    def __getattr__(self, name):
        if name in ("param", "grad", "s1", "s2"):
            return self.raw[name][CANARY:CANARY + self.n]
        raise AttributeError(name)

    def canaries_intact(self):
        for k, (name, raw) in enumerate(self.raw.items()):
            want = torch.full((CANARY,), 12345.0 + k, dtype=torch.float32, device=raw.device)
            if not (torch.equal(raw[:CANARY], want) and torch.equal(raw[CANARY + self.n:], want)):
                return False
        return True

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("param", "grad", "s1", "s2")}


def seg_table(bounds, active, missed, dev="cuda"):
    from mvlpt_amd import _lib
    host = (_lib.MvlptOptimSeg * len(bounds))()
    for s, (b, e), a, m in zip(host, bounds, active, missed):
        s.begin, s.end, s.active, s.missed = b, e, int(a), m
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)


def launch(kind, hyper, buf, segs_dev, n_segs, launch_no, loss=None, count_skips=True):
    from mvlpt_amd import _lib
    h = _lib.MvlptOptimHyper()
    h.kind, h.lr, h.weight_decay, h.launch = kind, hyper["lr"], hyper.get("weight_decay", 0.0), launch_no
    h.momentum, h.dampening, h.nesterov = hyper.get("momentum", 0.0), hyper.get("dampening", 0.0), int(hyper.get("nesterov", False))
    h.beta1, h.beta2, h.eps = hyper.get("beta1", 0.9), hyper.get("beta2", 0.999), hyper.get("eps", 1e-8)
    need1 = kind != R.SGD or hyper.get("momentum", 0.0) != 0
    rc = _lib.lib.mvlpt_op_optim_step(
        C.byref(h), buf.param.data_ptr(), buf.grad.data_ptr(), buf.s1.data_ptr() if need1 else None,
        buf.s2.data_ptr() if kind != R.SGD else None, buf.n, segs_dev.data_ptr(), n_segs, None if loss is None else loss.data_ptr(),
        buf.skipped.data_ptr() if count_skips else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, None, "op_optim_step")


def bounds_of(lengths):
    ends = np.cumsum(lengths).tolist()
    return list(zip([0] + ends[:-1], ends))


def check_step(kind, hyper, before, buf, bounds, active, steps_taken, what):
    """Every element of param / state1 / state2 against the float64 reference from `before` (the device's inputs of this step)."""
    h = as_f32(hyper)
    k = 8 if kind == R.SGD else 32
    b64 = {n: v.cpu().numpy().astype(np.float64) for n, v in before.items()}
    segs = [(b, e, a, t) for (b, e), a, t in zip(bounds, active, steps_taken)]
    has_buf = kind != R.SGD or h.get("momentum", 0.0) != 0
    P, S1, S2 = R.flat_step(kind, h, b64["param"], b64["grad"], b64["s1"] if has_buf else None, b64["s2"] if kind != R.SGD else None, segs)
    got = {n: getattr(buf, n).cpu().numpy().astype(np.float64) for n in ("param", "s1", "s2")}
    worst = {}
    for (b, e), a, t in zip(bounds, active, steps_taken):
        sl = slice(b, e)
        if not a:
            for n in ("param", "s1", "s2"):
                assert torch.equal(getattr(buf, n)[sl], before[n][sl]), f"{what}: inactive segment [{b}, {e}) of {n} was touched"
            continue
        if kind == R.SGD:
            Tp, Tb = R.sgd_terms(b64["param"][sl], b64["grad"][sl], b64["s1"][sl], t == 1, h["lr"], h["weight_decay"], h["momentum"],
                                 h["dampening"], h["nesterov"])
            pairs = [("param", P, Tp)] + ([("s1", S1, Tb)] if has_buf else [])
        else:
            Tp, Tm, Tv = R.adam_terms(b64["param"][sl], b64["grad"][sl], b64["s1"][sl], b64["s2"][sl], t, h["lr"], h["weight_decay"],
                                      h["beta1"], h["beta2"], h["eps"], kind == R.ADAMW)
            pairs = [("param", P, Tp), ("s1", S1, Tm), ("s2", S2, Tv)]
        for n, want, T in pairs:
            err = np.abs(got[n][sl] - want[sl])
            ratio = float((err / (U * T + 1e-300)).max())
            worst[n] = max(worst.get(n, 0.0), ratio)
            assert ratio <= k, f"{what}: {n} segment [{b}, {e}) is {ratio:.2f} * 2^-24 * T off (bound {k})"
        if kind == R.SGD and not has_buf:
            assert torch.equal(buf.s1[sl], before["s1"][sl])
    print(f"{what}: worst error / (2^-24 T) = " + ", ".join(f"{n} {v:.2f}" for n, v in worst.items()) + f" (bound {k})")
    assert buf.canaries_intact(), f"{what}: a canary next to a buffer changed"
    assert torch.equal(buf.grad, before["grad"])


def run_five_steps(kind, hyper, lengths, always_off, sits_out, late=None, seed=0):
    """5 consecutive launches: segments `always_off` never take part, `sits_out` misses steps 2-3 and returns (missed = 2), `late`
    (optional) takes its FIRST step at launch 3 (missed = 2: the first-step rule at a launch number other than 1)."""
    gen = torch.Generator().manual_seed(seed)
    bounds = bounds_of(lengths)
    n = bounds[-1][1]
    buf = Buffers(n, gen)
    steps = [0] * len(lengths)
    for launch_no in range(1, 6):
        active = [i not in always_off and not (i == sits_out and launch_no in (2, 3)) and not (i == late and launch_no < 3)
                  for i in range(len(lengths))]
        for i, a in enumerate(active):
            steps[i] += a
        missed = [launch_no - s if a else 0 for a, s in zip(active, steps)]
        buf.grad.copy_(torch.randn(n, generator=gen))
        before = buf.snapshot()
        launch(kind, as_f32(hyper), buf, seg_table(bounds, active, missed), len(bounds), launch_no)
        torch.cuda.synchronize()
        check_step(kind, hyper, before, buf, bounds, active, steps, f"kind {kind} {hyper} n={n} launch {launch_no}")
    assert int(buf.skipped.item()) == 0
    return buf


@pytest.mark.parametrize("hyper", SGD_HYPERS, ids=lambda h: "m{momentum}-wd{weight_decay}-d{dampening}-n{nesterov:d}".format(**h))
def test_sgd_main_layout(hyper):
    run_five_steps(R.SGD, hyper, MAIN_LENGTHS, always_off={2, 4}, sits_out=5)


@pytest.mark.parametrize("kind,hyper", ADAM_HYPERS, ids=lambda v: str(v["weight_decay"]) if isinstance(v, dict) else ["sgd", "adam", "adamw"][v])
def test_adam_main_layout(kind, hyper):
    run_five_steps(kind, hyper, MAIN_LENGTHS, always_off={2, 4}, sits_out=5)


@pytest.mark.parametrize("kind,hyper", [(R.SGD, SGD_HYPERS[1]), (R.SGD, SGD_HYPERS[3])] + ADAM_HYPERS[::2], ids=["sgd-nesterov", "sgd-m0", "adam", "adamw"])
def test_one_element_buffer(kind, hyper):
    run_five_steps(kind, hyper, [1], always_off=set(), sits_out=0)


@pytest.mark.parametrize("kind,hyper", [(R.SGD, SGD_HYPERS[0]), (R.SGD, SGD_HYPERS[2]), ADAM_HYPERS[0], ADAM_HYPERS[2]],
                         ids=["sgd", "sgd-dampening", "adam", "adamw"])
def test_upt4_tensor_list(kind, hyper):
    """The real UPT-4 tensor list (566 400 elements, 554 blocks): vpt_embeddings_deep sits out steps 2-3, the projection's first
    bias takes its first step at launch 3, ctx never has a gradient."""
    from tools.optim_bench import numel, upt4_shapes
    shapes = upt4_shapes()
    assert numel(shapes) == 566400
    run_five_steps(kind, hyper, [numel([s]) for s in shapes], always_off={2}, sits_out=1, late=4)


@pytest.mark.parametrize("kind,hyper", [(R.SGD, SGD_HYPERS[0]), ADAM_HYPERS[0], ADAM_HYPERS[2]], ids=["sgd", "adam", "adamw"])
def test_loss_guard(kind, hyper):
    """A non-finite loss: nothing is written and `skipped` goes up by exactly one per launch; a finite loss: a normal step.  The
    gradients are ordinary finite numbers throughout."""
    gen = torch.Generator().manual_seed(5)
    bounds = bounds_of(MAIN_LENGTHS)
    n = bounds[-1][1]
    buf = Buffers(n, gen)
    active, missed = [True] * len(bounds), [0] * len(bounds)
    segs = seg_table(bounds, active, missed)
    buf.grad.copy_(torch.randn(n, generator=gen))
    before = buf.snapshot()
    launch(kind, as_f32(hyper), buf, segs, len(bounds), 1, loss=torch.tensor([0.75], device="cuda"))
    torch.cuda.synchronize()
    assert int(buf.skipped.item()) == 0
    check_step(kind, hyper, before, buf, bounds, active, [1] * len(bounds), "finite loss")
    for k, bad in enumerate([float("nan"), float("inf"), float("-inf")]):
        buf.grad.copy_(torch.randn(n, generator=gen))
        before = buf.snapshot()
        launch(kind, as_f32(hyper), buf, segs, len(bounds), 2, loss=torch.tensor([bad], device="cuda"))
        torch.cuda.synchronize()
        assert int(buf.skipped.item()) == k + 1, f"loss {bad}: skipped = {int(buf.skipped.item())}"
        for name in ("param", "grad", "s1", "s2"):
            assert torch.equal(getattr(buf, name), before[name]), f"loss {bad}: {name} changed"
        assert buf.canaries_intact()
    launch(kind, as_f32(hyper), buf, segs, len(bounds), 2, loss=torch.tensor([float("nan")], device="cuda"), count_skips=False)   # no counter: still no write
    torch.cuda.synchronize()
    assert torch.equal(buf.param, before["param"]) and int(buf.skipped.item()) == 3
    before = buf.snapshot()
    launch(kind, as_f32(hyper), buf, segs, len(bounds), 2, loss=torch.tensor([3.0e38], device="cuda"))
    torch.cuda.synchronize()
    assert int(buf.skipped.item()) == 3
    check_step(kind, hyper, before, buf, bounds, active, [2] * len(bounds), "large finite loss")


def test_arguments_are_checked():
    from mvlpt_amd import _lib
    gen = torch.Generator().manual_seed(0)
    buf = Buffers(8, gen)
    segs = seg_table([(0, 8)], [True], [0])
    h = _lib.MvlptOptimHyper()
    h.kind, h.lr, h.launch = 0, 0.1, 1
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = _lib.lib.mvlpt_op_optim_step
    assert call(C.byref(h), buf.param.data_ptr() + 4, buf.grad.data_ptr(), None, None, 7, segs.data_ptr(), 1, None, None, s) == -1   # alignment
    assert call(C.byref(h), buf.param.data_ptr(), buf.grad.data_ptr(), None, None, 0, segs.data_ptr(), 1, None, None, s) == -1      # n
    h.kind = 1
    assert call(C.byref(h), buf.param.data_ptr(), buf.grad.data_ptr(), buf.s1.data_ptr(), None, 8, segs.data_ptr(), 1, None, None, s) == -1   # Adam without state2
    h.kind, h.launch = 0, 0
    assert call(C.byref(h), buf.param.data_ptr(), buf.grad.data_ptr(), None, None, 8, segs.data_ptr(), 1, None, None, s) == -1      # launch < 1
    h.launch = 1
    assert call(C.byref(h), buf.param.data_ptr(), buf.grad.data_ptr(), None, None, 8, segs.data_ptr(), 1025, None, None, s) == -4   # too many segments
    torch.cuda.synchronize()
    assert buf.canaries_intact()


def _fused_sgd(shapes, **hyper):
    from mvlpt_amd.distributed import FlatGradients, FlatParameters
    from mvlpt_amd.optim import FusedSGD
    gen = torch.Generator().manual_seed(1)
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen).cuda()) for s in shapes]
    fp, fg = FlatParameters(params), FlatGradients(params)
    return params, fp, fg, FusedSGD(fp, fg, **hyper), gen


def test_fused_sgd_bumps_the_version_counters():
    """The kernel writes behind autograd's back; step() bumps `_version` of every parameter it updated (model.py keys the evaluation
    text-feature cache on it) and of no other."""
    params, fp, fg, opt, gen = _fused_sgd([(3, 5), (7,), (2, 2)], lr=0.1, momentum=0.9)
    assert fp.intact() and all(p.is_leaf and isinstance(p, torch.nn.Parameter) for p in params)
    for i in (0, 2):
        params[i].grad = torch.randn(params[i].shape, generator=gen).cuda()
    v0 = [p._version for p in params]
    keep = params[1].detach().clone()
    before0 = params[0].detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert params[0]._version > v0[0] and params[2]._version > v0[2] and params[1]._version == v0[1]
    assert torch.equal(params[1].detach(), keep) and params[1].grad is None and params[1] not in opt.state
    assert not torch.equal(params[0].detach(), before0)
    assert fg.intact() and fp.intact()                         # step() adopted the hand-assigned gradients as views
    assert opt.state[params[0]]["momentum_buffer"].data_ptr() == opt._view1[0].data_ptr()
    # the same step by torch.optim.SGD from the same start
    ref = torch.nn.Parameter(before0.clone())
    ref.grad = params[0].grad.clone()
    torch.optim.SGD([ref], lr=0.1, momentum=0.9).step()
    assert float((ref.detach() - params[0].detach()).abs().max()) <= 8 * U * float((before0.abs() + 0.1 * ref.grad.abs()).max())


def test_fused_step_uploads_the_table_only_when_the_active_set_changes():
    params, fp, fg, opt, gen = _fused_sgd([(4,), (6,)], lr=0.1, momentum=0.9)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).cuda()
    opt.step()
    table = opt._segs_dev.clone()
    for _ in range(3):                                          # steady state: the device table is not written again
        opt.step()
        assert torch.equal(opt._segs_dev, table)
    params[1].grad = None
    opt.step()
    opt.step()
    params[1].grad = fg.views[1]
    opt.step()
    host = opt._segs_host
    assert (host[0].missed, host[1].missed, host[1].active) == (0, 2, 1) and opt._steps == [7, 5] and opt._launch == 7
    assert not torch.equal(opt._segs_dev, table)
