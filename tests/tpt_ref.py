"""Plain float64 reference of the test-time prompt tuning head (forward, selection, backward as include/mvlpt_hip.h states them), the
seeded inputs the GPU tests draw, and the bounds those tests hold the kernels to (tests/test_hip_tpt_head.py, tests/test_hip_tpt.py).
Nothing here touches the device: tests/test_tpt_ref.py pins the written-out gradient to torch autograd in float64, derives the bounds
from the error of a plain fp32 host implementation and checks the entropy gap at the selection boundary of every case."""
import math

import torch

TPT_SCALE = 100.0
# (G, V, C, e, k): the shapes of the kernel test
TPT_CASES = [(1, 1, 1, 64, 1), (1, 2, 2, 64, 1), (2, 5, 7, 128, 2), (4, 33, 65, 768, 3), (3, 64, 17, 512, 6), (2, 64, 257, 576, 6),
             (1, 64, 1000, 1024, 6), (1, 128, 2191, 512, 12), (2, 8, 9, 64, 8)]
# Seed offset per case: the first one for which (a) the float64 entropy gap at the selection boundary is at least 100 * 4e-5 *
# max(1, max H) (tests/test_tpt_ref.py::test_selection_gap asks for 100 * TPT_H_TOL) and (b) every image's loss is at least 1e-2.  With
# two classes at scale 100 nearly every draw is saturated: loss 1e-7, a gradient that is all cancellation and of which plain fp32
# keeps one digit.  Such a draw checks nothing, so the case is drawn again, not skipped.  Nothing else went into the choice.
TPT_SEED_SHIFT = {(1, 2, 2, 64, 1): 11, (2, 5, 7, 128, 2): 1, (3, 64, 17, 512, 6): 8}
# The tie cases (views 1 and 5 share their bits and sit at the selection boundary) and their seed offsets: the first for which every
# OTHER view's entropy is at least 100 * 4e-5 * max(1, max H) away from the pair's (test_tie_inputs_sit_at_the_boundary).
TPT_TIE_SEED_SHIFT = {(3, 64, 17, 512, 6): 14, (2, 8, 9, 64, 3): 0}

# Bounds: the error of a plain fp32 torch implementation of the same formulae (tpt_ref(dtype=torch.float32) below, the selection taken
# from float64) against float64 on the test's own inputs, times 4 (fast intrinsics and another summation order).  H and loss relative
# to max(1, |ref|), z and dtxt relative to max|ref|.  Measured on the CPU over TPT_CASES:
#   H     largest fp32 error 6.584e-6, at (1, 128, 2191, 512, 12) -> bound 2.63e-5
#   loss  largest fp32 error 5.703e-7, at (4, 33, 65, 768, 3)     -> bound 2.28e-6
#   z     largest fp32 error 6.446e-7, at (1, 64, 1000, 1024, 6)  -> bound 2.58e-6
#   dtxt  largest fp32 error 2.585e-5, at (2, 5, 7, 128, 2)       -> bound 1.03e-4   (the other cases: 1.7e-6 .. 9.6e-6)
# tests/test_tpt_ref.py::test_bounds_are_four_times_the_fp32_host_error re-measures them and holds the constants to the figures.
TPT_H_TOL = 2.63e-5
TPT_LOSS_TOL = 2.28e-6
TPT_DTXT_TOL = 1.03e-4
TPT_Z_TOL = 2.58e-6


def tpt_inputs(G, V, C, e, k, tie=False):
    """img [G, V, e] (x3), txt [G*C, e] (x0.02), w [G] in [0.5, 1.5).  tie: views 1 and 5 of every group get the same bits."""
    shift = TPT_TIE_SEED_SHIFT[(G, V, C, e, k)] if tie else TPT_SEED_SHIFT.get((G, V, C, e, k), 0)
    g = torch.Generator().manual_seed(100003 * G + 1009 * V + 31 * C + e + 7 * k + shift)
    img = torch.randn(G, V, e, generator=g) * 3
    txt = torch.randn(G * C, e, generator=g) * 0.02
    w = torch.rand(G, generator=g) + 0.5
    if tie:
        # Views 1 and 5 become copies of the view that has exactly k - 1 of the OTHER views in front of it, and that view itself a copy
        # of the least confident one: the pair sits at the selection boundary, view 1 is the k-th selected, view 5 the first left out.
        assert V >= max(7, k + 4)
        H = tpt_forward(img, txt, TPT_SCALE, k)[1]
        for q in range(G):
            rest = sorted((v for v in range(V) if v not in (1, 5)), key=lambda v: float(H[q, v]))
            src = rest[k - 1]
            img[q, 1] = img[q, src]
            img[q, 5] = img[q, src]
            img[q, src] = img[q, rest[-1]]
    return img, txt, w


def select(H, k):
    """[G, k] int64: the k smallest under (H, view index), NaN behind every number (a stable sort of H with NaN as +inf-and-beyond)."""
    G, V = H.shape
    key = torch.where(torch.isnan(H), torch.full_like(H, math.inf), H)
    nan = torch.isnan(H).to(torch.int64)
    out = []
    for g in range(G):
        order = sorted(range(V), key=lambda v: (int(nan[g, v]), float(key[g, v]), v))
        out.append(order[:k])
    return torch.tensor(out, dtype=torch.int64)


def tpt_forward(img, txt, scale, k, dtype=torch.float64, sel=None):
    """(z [G, V, C], H [G, V], sel [G, k], logp of the selected views [G, k, C], a [G, C], loss [G]) in `dtype`."""
    img, txt = img.to(dtype), txt.to(dtype)
    G, V, e = img.shape
    C = txt.shape[0] // G
    imn = img / (img * img).sum(-1, keepdim=True).sqrt()
    tn = (txt / (txt * txt).sum(-1, keepdim=True).sqrt()).view(G, C, e)
    z = scale * torch.einsum("gve,gce->gvc", imn, tn)
    m = z.max(-1, keepdim=True).values
    logp = z - (m + torch.log(torch.exp(z - m).sum(-1, keepdim=True)))
    H = -(torch.exp(logp) * logp).sum(-1)
    if sel is None:
        sel = select(H, k)
    lps = torch.gather(logp, 1, sel.view(G, k, 1).expand(G, k, C))
    mx = lps.max(1, keepdim=True).values
    a = (mx + torch.log(torch.exp(lps - mx).sum(1, keepdim=True))).squeeze(1) - math.log(k)
    loss = -(torch.exp(a) * a).sum(-1)
    return z, H, sel, lps, a, loss


def tpt_ref(img, txt, scale, k, w=None, dtype=torch.float64, sel=None):
    """The head written out: (loss [G], H [G, V], sel [G, k], dtxt [G*C, e], z [G, V, C]); dtxt is the gradient of sum_g w_g loss[g]
    with respect to the un-normalised text rows with the selection held constant."""
    z, H, sel, lps, a, loss = tpt_forward(img, txt, scale, k, dtype, sel)
    img, txt = img.to(dtype), txt.to(dtype)
    G, V, e = img.shape
    C = txt.shape[0] // G
    wg = torch.ones(G, dtype=dtype) if w is None else w.to(dtype)
    p = torch.exp(lps)                                              # [G, k, C]
    u = -(a + 1).unsqueeze(1)                                       # [G, 1, C]
    dz = (wg.view(G, 1, 1) / k) * p * (u - (p * u).sum(-1, keepdim=True))
    imn = img / (img * img).sum(-1, keepdim=True).sqrt()
    nt = (txt * txt).sum(-1, keepdim=True).sqrt()
    tn = txt / nt
    ims = torch.gather(imn, 1, sel.view(G, k, 1).expand(G, k, e))   # [G, k, e]
    dtn = scale * torch.einsum("gkc,gke->gce", dz, ims).reshape(G * C, e)
    dtxt = (dtn - (dtn * tn).sum(-1, keepdim=True) * tn) / nt
    return loss, H, sel, dtxt, z


def boundary_gap(H, k):
    """[G]: float64 gap between the k-th and the (k+1)-th smallest entropy (inf when every view is selected)."""
    G, V = H.shape
    if k >= V:
        return torch.full((G,), math.inf, dtype=torch.float64)
    s = H.double().sort(-1).values
    return s[:, k] - s[:, k - 1]


def rel_max1(a, b):
    """max |a - b| / max(1, |b|), elementwise, in float64."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b).abs() / b.abs().clamp(min=1.0)).max())


def rel(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
