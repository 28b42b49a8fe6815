"""The Tip-Adapter head at kernel level (-m gpu): mvlpt_op_tip_logits / _train_fwd / _train_bwd / _search against the float64 reference
and the bounds of tests/tip_ref.py.  Every output inside its bound (the largest error / bound ratio is printed per case), exact zeros,
empty classes, row independence, bit-equal reruns, the search counts bracketed by the decided rows and equal to tip_logits point by
point, guard regions and refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import tip_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                    # elements in front of and behind every buffer
SENT_F, SENT_I = -12345.0, -77


class Buf:
    """A device buffer of n elements between two guard regions filled with a sentinel."""

    def __init__(self, n, dtype=torch.float32):
        self.sent = SENT_F if dtype.is_floating_point else SENT_I
        self.full = torch.full((n + 2 * GUARD,), self.sent, device=DEV, dtype=dtype)
        self.t = self.full[GUARD:GUARD + n]

    def guards_intact(self):
        return bool((self.full[:GUARD] == self.sent).all()) and bool((self.full[-GUARD:] == self.sent).all())

    def untouched(self):
        return bool((self.full == self.sent).all())


def ws_bytes(N, NK, Cn, D, nb, na, mode):
    from mvlpt_amd import _lib
    out = C.c_int64()
    _lib.check(_lib.lib.mvlpt_tip_workspace_bytes(N, NK, Cn, D, nb, na, mode, C.byref(out)), None, "tip_workspace_bytes")
    assert out.value % 4 == 0
    return out.value


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The case's arrays, generated once and never modified; numpy for the reference."""
    N, D, counts = case
    return R.make_case(N, D, counts, R.SIGMA, R.case_seed(*case))


@functools.lru_cache(maxsize=None)
def device_inputs(case):
    c = inputs(case)
    return {k: torch.from_numpy(c[k]).to(DEV).contiguous() for k in ("F", "y", "K", "key_ptr", "W")}


@functools.lru_cache(maxsize=None)
def reference(case, alpha, beta):
    c = inputs(case)
    return R.train_bounds(c["F"], c["y"], c["K"], c["key_ptr"], c["key_cls"], c["W"], alpha, beta)


def sizes(d):
    return d["F"].shape[0], d["K"].shape[0], d["W"].shape[0], d["F"].shape[1]


def tip_logits(d, alpha, beta, rows=None):
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    F = d["F"] if rows is None else d["F"][rows].contiguous()
    N, (_, NK, Cn, D) = F.shape[0], sizes(d)
    out = Buf(N * Cn)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib.mvlpt_op_tip_logits(_ptr(F), _ptr(d["K"]), _ptr(d["key_ptr"]), _ptr(d["W"]), R.SCALE, alpha, beta, N, NK, Cn, D,
                                                _ptr(out.t), _stream()), None, "op_tip_logits")
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.t.view(N, Cn).cpu().numpy()


def tip_train(d, alpha, beta, want_logits=True, bwd=True):
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    N, NK, Cn, D = sizes(d)
    nb = ws_bytes(N, NK, Cn, D, 0, 0, _lib.TIP_TRAIN)
    ws, loss, correct, dK = Buf(nb // 4), Buf(1), Buf(1, torch.int32), Buf(NK * D)
    z = Buf(N * Cn) if want_logits else None
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib.mvlpt_op_tip_train_fwd(_ptr(d["F"]), _ptr(d["y"]), _ptr(d["K"]), _ptr(d["key_ptr"]), _ptr(d["W"]), R.SCALE,
                                                   alpha, beta, N, NK, Cn, D, _ptr(loss.t), _ptr(correct.t), _ptr(z.t) if z else None,
                                                   _ptr(ws.t), nb, _stream()), None, "op_tip_train_fwd")
        if bwd:
            _lib.check(_lib.lib.mvlpt_op_tip_train_bwd(_ptr(d["F"]), alpha, beta, N, NK, Cn, D, _ptr(dK.t), _ptr(ws.t), nb, _stream()),
                       None, "op_tip_train_bwd")
    torch.cuda.synchronize()
    for b in (ws, loss, correct, dK) + ((z,) if z else ()):
        assert b.guards_intact()
    if not bwd:
        assert dK.untouched()
    return {"loss": float(loss.t.cpu()[0]), "correct": int(correct.t.cpu()[0]), "dK": dK.t.view(NK, D).cpu().numpy(),
            "z": z.t.view(N, Cn).cpu().numpy() if z else None}


def tip_search(d, betas, alphas, rows=None):
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    F, y = (d["F"], d["y"]) if rows is None else (d["F"][rows].contiguous(), d["y"][rows].contiguous())
    N, (_, NK, Cn, D) = F.shape[0], sizes(d)
    b_d, a_d = torch.tensor(betas, dtype=torch.float32, device=DEV), torch.tensor(alphas, dtype=torch.float32, device=DEV)
    nb, na = len(betas), len(alphas)
    nbytes = ws_bytes(N, NK, Cn, D, nb, na, _lib.TIP_SEARCH)
    ws, counts = Buf(nbytes // 4), Buf(nb * na, torch.int32)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib.mvlpt_op_tip_search(_ptr(F), _ptr(y), _ptr(d["K"]), _ptr(d["key_ptr"]), _ptr(d["W"]), R.SCALE, _ptr(b_d), _ptr(a_d),
                                                N, NK, Cn, D, nb, na, _ptr(counts.t), _ptr(ws.t), nbytes, _stream()), None, "op_tip_search")
    torch.cuda.synchronize()
    assert ws.guards_intact() and counts.guards_intact()
    return counts.t.view(nb, na).cpu().numpy()


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(err / np.maximum(bound, 1e-300))) if np.size(err) else 0.0


def f32(x):
    return np.float32(x)


@pytest.mark.parametrize("hp", R.HEAD_HPARAMS, ids=str)
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{len(c[2])}")
def test_head_against_float64(case, hp):
    alpha, beta = hp
    d, c, b = device_inputs(case), inputs(case), reference(case, alpha, beta)
    ref = b["ref"]
    z = tip_logits(d, alpha, beta)
    got = tip_train(d, alpha, beta)
    figs = {"z": ratio(z, ref["z"], b["z"]), "loss": abs(got["loss"] - ref["loss"]) / b["loss"], "dK": ratio(got["dK"], ref["dK"], b["dK"])}
    print(case[:2], len(case[2]), hp, "error / bound:", " ".join(f"{n} {v:.3f}" for n, v in figs.items()))
    assert np.array_equal(z, got["z"])                                   # one forward kernel: the train logits are the logits
    assert max(figs.values()) <= 1.0, figs
    ok = R.decided(ref["z"], b["z"])
    hit = ref["z"].argmax(1) == c["y"]
    assert (hit & ok).sum() <= got["correct"] <= (hit & ok).sum() + (~ok).sum()
    assert got["correct"] == int((z.argmax(1) == c["y"]).sum())           # ties to the lowest class, as numpy
    # without the optional output: the same bits
    again = tip_train(d, alpha, beta, want_logits=False)
    assert again["loss"] == got["loss"] and again["correct"] == got["correct"] and np.array_equal(again["dK"], got["dK"])
    if beta == 0.0:
        # every affinity is exp(0) = 1: the cache term is exactly alpha n_c, joined to the zero-shot logit by one fp32 addition
        z0 = tip_logits(d, 0.0, 0.0)
        n_c = np.diff(c["key_ptr"]).astype(np.float32)
        assert np.array_equal(z, z0 + f32(alpha) * n_c[None, :])
        assert not got["dK"].any()


def test_alpha_zero_has_no_gradient():
    case = R.HEAD_CASES[1]
    got = tip_train(device_inputs(case), 0.0, 5.5)
    assert not got["dK"].any()
    assert np.array_equal(got["z"], tip_logits(device_inputs(case), 0.0, 1.0))       # and beta no longer matters


def test_one_class_gives_exact_zeros():
    case = (5, 64, (3,))
    got = tip_train(device_inputs(case), 1.0, 5.5)
    assert got["loss"] == 0.0 and got["correct"] == 5 and not got["dK"].any()


def test_empty_class_is_the_zero_shot_logit():
    case = R.HEAD_CASES[1]
    empty = [i for i, n in enumerate(case[2]) if n == 0]
    assert empty
    d = device_inputs(case)
    z, z0 = tip_logits(d, 3.0, 7.0), tip_logits(d, 0.0, 7.0)
    assert np.array_equal(z[:, empty].view(np.int32), z0[:, empty].view(np.int32))
    full = [i for i, n in enumerate(case[2]) if n > 0]
    assert (z[:, full] > z0[:, full]).all()


@pytest.mark.parametrize("case", [R.HEAD_CASES[1], R.HEAD_CASES[3]], ids=lambda c: f"{c[0]}x{c[1]}")
def test_rows_do_not_depend_on_the_batch(case):
    d = device_inputs(case)
    z = tip_logits(d, 1.0, 5.5)
    rows = torch.arange(5, min(case[0], 200) - 3, 3, device=DEV)          # another row block, another position in it
    part = tip_logits(d, 1.0, 5.5, rows=rows)
    assert np.array_equal(part.view(np.int32), z[rows.cpu().numpy()].view(np.int32))
    one = tip_logits(d, 1.0, 5.5, rows=torch.tensor([case[0] - 1], device=DEV))
    assert np.array_equal(one.view(np.int32), z[-1:].view(np.int32))


def test_reruns_are_bit_equal():
    case = R.HEAD_CASES[2]
    d = device_inputs(case)
    a, b = tip_train(d, 1.0, 5.5), tip_train(d, 1.0, 5.5)
    assert a["loss"] == b["loss"] and a["correct"] == b["correct"]
    assert np.array_equal(a["z"].view(np.int32), b["z"].view(np.int32)) and np.array_equal(a["dK"].view(np.int32), b["dK"].view(np.int32))
    assert np.array_equal(tip_logits(d, 1.0, 5.5).view(np.int32), tip_logits(d, 1.0, 5.5).view(np.int32))
    assert np.array_equal(tip_search(d, R.SEARCH_BETAS, R.SEARCH_ALPHAS), tip_search(d, R.SEARCH_BETAS, R.SEARCH_ALPHAS))


@functools.lru_cache(maxsize=None)
def search_reference(case, betas, alphas):
    c = inputs(case)
    return R.search(c["F"], c["y"], c["K"], c["key_ptr"], c["W"], np.float32(betas), np.float32(alphas))


@pytest.mark.parametrize("case", R.SEARCH_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{len(c[2])}")
def test_search_counts(case):
    d, c = device_inputs(case), inputs(case)
    ref = search_reference(case, R.SEARCH_BETAS, R.SEARCH_ALPHAS)
    counts = tip_search(d, R.SEARCH_BETAS, R.SEARCH_ALPHAS)
    print(case[:2], "counts", counts.min(), "..", counts.max(), "undecided rows at most", ref["undecided"].max())
    assert (ref["sure"] <= counts).all() and (counts <= ref["sure"] + ref["undecided"]).all()
    if not ref["undecided"].any():
        assert np.array_equal(counts, ref["counts"])
        for b, beta in enumerate(R.SEARCH_BETAS):          # and the search is tip_logits at every grid point, one by one
            for a, alpha in enumerate(R.SEARCH_ALPHAS):
                z = tip_logits(d, float(f32(alpha)), float(f32(beta)))
                assert counts[b, a] == int((z.argmax(1) == c["y"]).sum()), (beta, alpha)


def test_search_published_grid():
    case = R.SEARCH_CASES[0]
    betas, alphas = R.published_grid()
    betas, alphas = tuple(float(f32(x)) for x in betas), tuple(float(f32(x)) for x in alphas)
    ref = search_reference(case, betas, alphas)
    counts = tip_search(device_inputs(case), betas, alphas)
    assert counts.shape == (200, 20)
    assert (ref["sure"] <= counts).all() and (counts <= ref["sure"] + ref["undecided"]).all()
    assert R.winner(counts) == R.winner(ref["counts"]) or ref["undecided"].any()


def test_search_row_chunks_add_up():
    """131 classes x 200 betas make a row chunk of 4 992 rows: 5 100 rows take two chunks.  A row's logits do not depend on the rows
    around it, so the counts are those of the two chunks searched alone."""
    from mvlpt_amd import _lib
    case = (5100, 68, (2,) * 130 + (1,))
    d = device_inputs(case)
    betas, alphas = R.published_grid()
    betas, alphas = tuple(float(f32(x)) for x in betas), tuple(float(f32(x)) for x in alphas)
    chunk = ((512 << 20) // (131 * 201 * 4)) // 128 * 128
    assert chunk == 4992 < case[0]
    assert ws_bytes(case[0], 261, 131, 68, 200, 20, _lib.TIP_SEARCH) == ws_bytes(chunk, 261, 131, 68, 200, 20, _lib.TIP_SEARCH)
    whole = tip_search(d, betas, alphas)
    head = tip_search(d, betas, alphas, rows=torch.arange(0, chunk, device=DEV))
    tail = tip_search(d, betas, alphas, rows=torch.arange(chunk, case[0], device=DEV))
    assert np.array_equal(whole, head + tail)
    assert whole.max() <= case[0] and len(np.unique(whole)) > 1


def test_workspace_at_imagenet_size_stays_under_a_gibibyte():
    from mvlpt_amd import _lib
    for D in (512, 1024):
        assert ws_bytes(50000, 16000, 1000, D, 200, 20, _lib.TIP_SEARCH) < (1 << 30)
    assert ws_bytes(256, 16000, 1000, 1024, 0, 0, _lib.TIP_TRAIN) < (1 << 26)
    assert ws_bytes(256, 16000, 1000, 1024, 0, 0, _lib.TIP_LOGITS) == 0


def test_refusals_return_err_arg_and_write_nothing():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    lib = _lib.lib
    N, NK, Cn, D, nb, na = 9, 12, 5, 64, 3, 2
    F, K, W = torch.randn(N, D, device=DEV), torch.randn(NK, D, device=DEV), torch.randn(Cn, D, device=DEV)
    y = torch.zeros(N, dtype=torch.int32, device=DEV)
    kp = torch.tensor([0, 2, 4, 4, 9, 12], dtype=torch.int32, device=DEV)
    be, al = torch.ones(nb, device=DEV), torch.ones(na, device=DEV)
    wt, wsr = ws_bytes(N, NK, Cn, D, 0, 0, _lib.TIP_TRAIN), ws_bytes(N, NK, Cn, D, nb, na, _lib.TIP_SEARCH)
    bufs = {"ws": Buf(max(wt, wsr) // 4), "z": Buf(N * Cn), "loss": Buf(1), "correct": Buf(1, torch.int32), "dK": Buf(NK * D),
            "counts": Buf(nb * na, torch.int32)}

    def args(**over):
        a = dict(N=N, NK=NK, C=Cn, D=D, nb=nb, na=na, train_bytes=wt, search_bytes=wsr,
                 ptr=dict(F=F, K=K, kp=kp, W=W, y=y, be=be, al=al, ws=bufs["ws"].t, z=bufs["z"].t, loss=bufs["loss"].t,
                          correct=bufs["correct"].t, dK=bufs["dK"].t, counts=bufs["counts"].t))
        for k, v in over.items():
            if k in a["ptr"]:
                a["ptr"][k] = v
            else:
                a[k] = v
        return a

    every = ("logits", "fwd", "bwd", "search")
    # (override, the entries it must stop).  The sizes named below never exceed what the buffers hold unless the call is refused.
    bad = [(dict(N=0), every), (dict(NK=0), every), (dict(C=0), every), (dict(C=_lib.TIP_MAX_CLASSES + 1), every), (dict(D=0), every),
           (dict(D=62), every), (dict(nb=0), ("search",)), (dict(na=0), ("search",)), (dict(nb=_lib.TIP_MAX_NB + 1), ("search",)),
           (dict(na=_lib.TIP_MAX_NA + 1), ("search",)), (dict(train_bytes=wt - 1), ("fwd", "bwd")), (dict(search_bytes=wsr - 1), ("search",)),
           (dict(train_bytes=0, search_bytes=0), ("fwd", "bwd", "search")), (dict(train_bytes=-1, search_bytes=-1), ("fwd", "bwd", "search")),
           (dict(ws=None), ("fwd", "bwd", "search")), (dict(F=None), every), (dict(K=None), ("logits", "fwd", "search")),
           (dict(kp=None), ("logits", "fwd", "search")), (dict(W=None), ("logits", "fwd", "search")), (dict(y=None), ("fwd", "search")),
           (dict(be=None), ("search",)), (dict(al=None), ("search",)), (dict(loss=None), ("fwd",)), (dict(correct=None), ("fwd",)),
           (dict(dK=None), ("bwd",)), (dict(counts=None), ("search",))]
    out = C.c_int64(-5)
    with torch.cuda.device(DEV):
        for over, stopped in bad:
            a = args(**over)
            # only the entries that must refuse are called
            p = {k: _ptr(v) for k, v in a["ptr"].items()}
            s = _stream()
            for name in stopped:
                if name == "logits":
                    rc = lib.mvlpt_op_tip_logits(p["F"], p["K"], p["kp"], p["W"], 100.0, 1.0, 5.5, a["N"], a["NK"], a["C"], a["D"], p["z"], s)
                elif name == "fwd":
                    rc = lib.mvlpt_op_tip_train_fwd(p["F"], p["y"], p["K"], p["kp"], p["W"], 100.0, 1.0, 5.5, a["N"], a["NK"], a["C"], a["D"],
                                                    p["loss"], p["correct"], p["z"], p["ws"], a["train_bytes"], s)
                elif name == "bwd":
                    rc = lib.mvlpt_op_tip_train_bwd(p["F"], 1.0, 5.5, a["N"], a["NK"], a["C"], a["D"], p["dK"], p["ws"], a["train_bytes"], s)
                else:
                    rc = lib.mvlpt_op_tip_search(p["F"], p["y"], p["K"], p["kp"], p["W"], 100.0, p["be"], p["al"], a["N"], a["NK"], a["C"],
                                                 a["D"], a["nb"], a["na"], p["counts"], p["ws"], a["search_bytes"], s)
                assert rc == _lib.ERR_ARG and _lib.last_error(None), (over, name)
            if set(over) & {"N", "NK", "C", "D"}:
                for mode in (_lib.TIP_LOGITS, _lib.TIP_TRAIN, _lib.TIP_SEARCH):
                    assert lib.mvlpt_tip_workspace_bytes(a["N"], a["NK"], a["C"], a["D"], nb, na, mode, C.byref(out)) == _lib.ERR_ARG
            if set(over) & {"nb", "na"}:
                assert lib.mvlpt_tip_workspace_bytes(N, NK, Cn, D, a["nb"], a["na"], _lib.TIP_SEARCH, C.byref(out)) == _lib.ERR_ARG
            assert out.value == -5
        assert lib.mvlpt_op_tip_logits(_ptr(F), _ptr(K), _ptr(kp), _ptr(W), 100.0, 1.0, 5.5, N, NK, Cn, D, None, _stream()) == _lib.ERR_ARG
        assert lib.mvlpt_tip_workspace_bytes(N, NK, Cn, D, nb, na, 3, C.byref(out)) == _lib.ERR_ARG
        assert lib.mvlpt_tip_workspace_bytes(N, NK, Cn, D, nb, na, _lib.TIP_SEARCH, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for n, b in bufs.items():
        assert b.untouched(), n


def test_engine_binding_and_state_rule():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    eng = Engine(ARCHS["tiny"], device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="tip_train_bwd without tip_train_fwd"):
        eng.tip_train_bwd()
    case, (alpha, beta) = R.HEAD_CASES[1], R.HEAD_HPARAMS[0]
    d, b = device_inputs(case), reference(case, alpha, beta)
    a = (d["K"], d["key_ptr"], d["W"], R.SCALE)
    z = eng.tip_logits(d["F"], *a, alpha, beta)
    assert np.array_equal(z.cpu().numpy(), tip_logits(d, alpha, beta))
    loss, correct = eng.tip_train_fwd(d["F"], d["y"], *a, alpha, beta)
    dK = eng.tip_train_bwd()
    ws = eng._tip_ws
    direct = tip_train(d, alpha, beta)
    assert float(loss) == direct["loss"] and int(correct) == direct["correct"] and np.array_equal(dK.cpu().numpy(), direct["dK"])
    assert ratio(dK.cpu().numpy(), b["ref"]["dK"], b["dK"]) <= 1.0
    out = eng.tip_train_fwd(d["F"], d["y"], *a, alpha, beta, want_logits=True)
    assert len(out) == 3 and np.array_equal(out[2].cpu().numpy(), direct["z"]) and eng._tip_ws is ws        # grow-only: reused
    counts = eng.tip_search(d["F"], d["y"], *a, torch.tensor(R.SEARCH_BETAS, device=DEV), torch.tensor(R.SEARCH_ALPHAS, device=DEV))
    assert np.array_equal(counts.cpu().numpy(), tip_search(d, R.SEARCH_BETAS, R.SEARCH_ALPHAS))
    with pytest.raises(RuntimeError, match="tip_train_bwd without tip_train_fwd"):      # the search took the workspace
        eng.tip_train_bwd()
    eng.tip_train_fwd(d["F"], d["y"], *a, alpha, beta)
    with pytest.raises(RuntimeError):                                 # a refused forward leaves no state behind
        eng.tip_train_fwd(d["F"][:, :62], d["y"], d["K"][:, :62], d["key_ptr"], d["W"][:, :62], R.SCALE, alpha, beta)
    with pytest.raises(RuntimeError, match="tip_train_bwd without tip_train_fwd"):
        eng.tip_train_bwd()
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        eng.tip_logits(d["F"].cpu(), *a, alpha, beta)
    with pytest.raises(ValueError, match="key_ptr"):
        eng.tip_logits(d["F"], d["K"], d["key_ptr"][:-1], d["W"], R.SCALE, alpha, beta)
    eng.close()
