"""Pins tests/optim_ref.py — the float64 reference the GPU tests of the fused optimizer step compare with — against
torch.optim.SGD / Adam / AdamW run in float64 on the CPU: 4 steps, one parameter without a gradient on steps 2-3 (torch skips it:
no decay, no momentum decay, its step count stands still), agreement to 1e-13 of each tensor's largest magnitude."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

SHAPES = [(5,), (3, 4), (2, 3)]
STEPS = 4
SITS_OUT = {1: (1, 2)}          # parameter 1 has grad None on steps 2-3 (0-based 1, 2)

SGD_CASES = [
    dict(lr=0.05, momentum=0.9, weight_decay=5e-4, dampening=0.0, nesterov=False),
    dict(lr=0.05, momentum=0.9, weight_decay=5e-4, dampening=0.0, nesterov=True),
    dict(lr=0.05, momentum=0.9, weight_decay=0.0, dampening=0.1, nesterov=False),
    dict(lr=0.05, momentum=0.0, weight_decay=5e-4, dampening=0.0, nesterov=False),
    dict(lr=0.05, momentum=0.0, weight_decay=0.0, dampening=0.0, nesterov=False),
    dict(lr=0.002, momentum=0.9, weight_decay=0.0, dampening=0.0, nesterov=True),
]
ADAM_CASES = [
    (R.ADAM, dict(lr=0.01, weight_decay=0.0)), (R.ADAM, dict(lr=0.01, weight_decay=5e-4)),
    (R.ADAMW, dict(lr=0.01, weight_decay=0.0)), (R.ADAMW, dict(lr=0.01, weight_decay=5e-4)), (R.ADAMW, dict(lr=0.01, weight_decay=1e-2)),
]


def _run(kind, hyper):
    rng = np.random.default_rng(7)
    init = [rng.standard_normal(s) for s in SHAPES]
    grads = [[rng.standard_normal(s) for s in SHAPES] for _ in range(STEPS)]
    for i, steps in SITS_OUT.items():
        for k in steps:
            grads[k][i] = None
    tp = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in init]
    if kind == R.SGD:
        opt = torch.optim.SGD(tp, **hyper)
    else:
        opt = (torch.optim.AdamW if kind == R.ADAMW else torch.optim.Adam)(tp, **hyper)
    ref = R.FlatOptimizer(kind, init, **hyper)
    for k in range(STEPS):
        for p, g in zip(tp, grads[k]):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        opt.step()
        ref.step(grads[k])
        for i, p in enumerate(tp):
            _close(ref.params[i], p.detach().numpy(), f"step {k + 1} param {i}")
            st = opt.state.get(p, {})
            if kind == R.SGD:
                if st.get("momentum_buffer") is not None:
                    _close(ref.s1[i], st["momentum_buffer"].numpy(), f"step {k + 1} momentum_buffer {i}")
            elif st:
                assert int(st["step"]) == ref.steps[i]
                _close(ref.s1[i], st["exp_avg"].numpy(), f"step {k + 1} exp_avg {i}")
                _close(ref.s2[i], st["exp_avg_sq"].numpy(), f"step {k + 1} exp_avg_sq {i}")
    assert ref.steps == [STEPS, STEPS - 2, STEPS]


def _close(a, b, what):
    err = float(np.abs(a - b).max()) / float(np.abs(b).max())
    assert err <= 1e-13, f"{what}: {err:.2e}"


@pytest.mark.parametrize("hyper", SGD_CASES, ids=lambda h: "m{momentum}-wd{weight_decay}-d{dampening}-n{nesterov:d}-lr{lr}".format(**h))
def test_sgd_reference_is_torch_sgd(hyper):
    _run(R.SGD, hyper)


@pytest.mark.parametrize("kind,hyper", ADAM_CASES, ids=lambda v: v["weight_decay"] if isinstance(v, dict) else ["sgd", "adam", "adamw"][v])
def test_adam_reference_is_torch_adam(kind, hyper):
    _run(kind, hyper)


def test_a_parameter_that_sat_out_was_not_touched():
    """torch skips a parameter with grad None altogether; so does the reference (its values after steps 2-3 are those after step 1)."""
    rng = np.random.default_rng(1)
    ref = R.FlatOptimizer(R.SGD, [rng.standard_normal(4), rng.standard_normal(3)], lr=0.1, momentum=0.9, weight_decay=5e-4)
    ref.step([rng.standard_normal(4), rng.standard_normal(3)])
    p1, b1 = ref.params[1].copy(), ref.s1[1].copy()
    ref.step([rng.standard_normal(4), None])
    assert np.array_equal(ref.params[1], p1) and np.array_equal(ref.s1[1], b1) and ref.steps == [2, 1]


def test_flat_step_leaves_uncovered_and_inactive_elements():
    rng = np.random.default_rng(2)
    p, g, m, v = rng.standard_normal(10), rng.standard_normal(10), rng.standard_normal(10), rng.random(10)
    P, M, V = R.flat_step(R.ADAM, dict(lr=0.01), p, g, m, v, [(0, 3, 1, 1), (3, 6, 0, 2), (7, 10, 1, 3)])
    assert np.array_equal(P[3:7], p[3:7]) and np.array_equal(M[3:7], m[3:7]) and np.array_equal(V[3:7], v[3:7])
    assert not np.array_equal(P[:3], p[:3]) and not np.array_equal(P[7:], p[7:])
    want, _, _ = R.adam(p[7:], g[7:], m[7:], v[7:], 3, 0.01)
    assert np.array_equal(P[7:], want)
