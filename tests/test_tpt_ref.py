"""CPU checks of tests/tpt_ref.py: the written-out head is pinned to torch autograd in float64, the bounds the GPU tests use are
derived from the error of a plain fp32 host implementation, and every case of the kernel test has a float64 entropy gap at the
selection boundary of at least 100 x the H bound, so a differing selection on the device is a failure and not a near-tie.  No GPU."""
import math

import pytest
import torch

from tests import tpt_ref as R

TIE_CASES = list(R.TPT_TIE_SEED_SHIFT)


def _autograd(img, txt, scale, sel, w):
    """sum_g w_g loss[g] through torch ops in float64 with the selection held constant; returns (loss [G], H [G, V], d txt)."""
    G, V, e = img.shape
    C = txt.shape[0] // G
    k = sel.shape[1]
    t64 = txt.double().requires_grad_(True)
    i64 = img.double()
    z = scale * torch.einsum("gve,gce->gvc", i64 / i64.norm(dim=-1, keepdim=True), (t64 / t64.norm(dim=-1, keepdim=True)).view(G, C, e))
    logp = torch.log_softmax(z, dim=-1)
    H = -(logp.exp() * logp).sum(-1)
    lps = torch.gather(logp, 1, sel.view(G, k, 1).expand(G, k, C))
    a = torch.logsumexp(lps, dim=1) - math.log(k)
    loss = -(a.exp() * a).sum(-1)
    (loss * w.double()).sum().backward()
    return loss.detach(), H.detach(), t64.grad


@pytest.mark.parametrize("case", [c for c in R.TPT_CASES if c[2] <= 300])
def test_ref_is_autograd(case):
    G, V, C, e, k = case
    img, txt, w = R.tpt_inputs(*case)
    loss, H, sel, dtxt, z = R.tpt_ref(img, txt, R.TPT_SCALE, k, w)
    l2, H2, g2 = _autograd(img, txt, R.TPT_SCALE, sel, w)
    assert R.rel_max1(loss, l2) <= 1e-13 and R.rel_max1(H, H2) <= 1e-13
    # 1e-10, not 1e-13: u - sum p u cancels where a view is confident, in float64 as anywhere
    assert float((dtxt - g2).abs().max()) <= 1e-10 * max(float(g2.abs().max()), 1e-300)
    assert sel.shape == (G, k) and all(len(set(r)) == k for r in sel.tolist())
    if C == 1:
        assert float(loss.abs().max()) == 0.0 and float(dtxt.abs().max()) == 0.0 and float(H.abs().max()) == 0.0
    # no weights = weights of 1
    d1 = R.tpt_ref(img, txt, R.TPT_SCALE, k, None)[3]
    assert torch.equal(d1, R.tpt_ref(img, txt, R.TPT_SCALE, k, torch.ones(G))[3])


def test_select_orders_by_entropy_then_index_nan_last():
    H = torch.tensor([[0.5, 0.25, float("nan"), 0.25, 0.0, float("inf"), 0.25]], dtype=torch.float64)
    assert R.select(H, 7).tolist() == [[4, 1, 3, 6, 0, 5, 2]]
    assert R.select(H, 2).tolist() == [[4, 1]]
    assert R.select(torch.full((1, 3), float("nan")), 2).tolist() == [[0, 1]]


@pytest.mark.parametrize("case", R.TPT_CASES)
def test_selection_gap(case):
    """Every non-tie case: the float64 gap between the k-th and (k+1)-th smallest entropy is at least 100 x the H bound."""
    G, V, C, e, k = case
    img, txt, _ = R.tpt_inputs(*case)
    H = R.tpt_forward(img, txt, R.TPT_SCALE, k)[1]
    gap = R.boundary_gap(H, k)
    scale = H.abs().max().clamp(min=1.0)
    assert float(gap.min()) >= 100 * R.TPT_H_TOL * float(scale), (case, float(gap.min()))
    if k == V:
        assert R.select(H, k).sort(-1).values.tolist() == [list(range(V))] * G


@pytest.mark.parametrize("case", TIE_CASES)
def test_tie_inputs_sit_at_the_boundary(case):
    G, V, C, e, k = case
    img, txt, _ = R.tpt_inputs(*case, tie=True)
    assert torch.equal(img[:, 1], img[:, 5])
    H = R.tpt_forward(img, txt, R.TPT_SCALE, k)[1]
    H[:, 5] = H[:, 1]                         # the same rows: one value, whatever the host's blocked product made of them
    sel = R.select(H, k)
    for g in range(G):
        assert int(sel[g, k - 1]) == 1 and 5 not in sel[g].tolist()
        others = torch.cat([H[g, :1], H[g, 2:5], H[g, 6:]])
        d = (others - H[g, 1]).abs().min()
        assert float(d) >= 100 * R.TPT_H_TOL * max(1.0, float(H[g].abs().max())), (case, g, float(d))


def _fp32_errors():
    worst = {"H": (0.0, None), "loss": (0.0, None), "dtxt": (0.0, None), "z": (0.0, None)}
    for case in R.TPT_CASES:
        G, V, C, e, k = case
        img, txt, w = R.tpt_inputs(*case)
        loss, H, sel, dtxt, z = R.tpt_ref(img, txt, R.TPT_SCALE, k, w)
        l32, H32, _, d32, z32 = R.tpt_ref(img, txt, R.TPT_SCALE, k, w, dtype=torch.float32, sel=sel)
        errs = {"H": R.rel_max1(H32, H), "loss": R.rel_max1(l32, loss), "z": R.rel(z32, z),
                "dtxt": R.rel(d32, dtxt) if float(dtxt.abs().max()) > 0 else 0.0}
        for name, v in errs.items():
            if v > worst[name][0]:
                worst[name] = (v, case)
    return worst


def test_bounds_are_four_times_the_fp32_host_error():
    """The four bounds are 4 x the error of plain fp32 torch against float64 on the GPU test's own inputs (tpt_ref.py records the
    figures).  An fp32 sum may be ordered differently on another host, so the constants are held to the re-measured error within a
    factor of 1.5 either way, not to the digit."""
    worst = _fp32_errors()
    print("fp32 host error: " + ", ".join(f"{n} {v:.3e} at {c}" for n, (v, c) in worst.items()))
    for name, tol in (("H", R.TPT_H_TOL), ("loss", R.TPT_LOSS_TOL), ("dtxt", R.TPT_DTXT_TOL), ("z", R.TPT_Z_TOL)):
        err = worst[name][0]
        assert 4 * err / 1.5 <= tol <= 4 * err * 1.5, (name, err, worst[name][1])
