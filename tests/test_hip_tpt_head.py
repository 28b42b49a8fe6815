"""The test-time prompt tuning head at kernel level (-m gpu): mvlpt_op_tpt_head_fwd / _bwd against the float64 reference of
tests/tpt_ref.py.  H, loss, dtxt and the optional z inside the bounds derived there (4 x the error of plain fp32 torch); the selection
equal to the reference's including its order, under the entropy gap tests/test_tpt_ref.py asserts on the CPU; exact zeros, exact ties,
group independence, bit-equal reruns, guard regions and refusals."""
import ctypes as C
import functools

import pytest
import torch

from tests import tpt_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                    # elements in front of and behind every buffer
SENT_F, SENT_I = -12345.0, -77
IDS = [str(c) for c in R.TPT_CASES]


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


def call(img, txt, k, w=None, want_z=False, scale=R.TPT_SCALE, bwd=True):
    """One forward (+ backward) through the C entries with guarded buffers; returns a dict of CPU tensors."""
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream, tpt_workspace_bytes
    G, V, e = img.shape
    Cn = txt.shape[0] // G
    img_d, txt_d = img.to(DEV).contiguous(), txt.to(DEV).contiguous()
    nb = tpt_workspace_bytes(G, V, Cn, e, k)
    assert nb % 4 == 0
    ws, loss, H, sel = Buf(nb // 4), Buf(G), Buf(G * V), Buf(G * k, torch.int32)
    z = Buf(G * V * Cn) if want_z else None
    dtxt = Buf(G * Cn * e)
    w_d = None if w is None else w.to(DEV).float().contiguous()
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib.mvlpt_op_tpt_head_fwd(_ptr(img_d), _ptr(txt_d), scale, G, V, Cn, e, k, _ptr(loss.t), _ptr(H.t), _ptr(sel.t),
                                                  _ptr(z.t) if z else None, _ptr(ws.t), nb, _stream()), None, "op_tpt_head_fwd")
        if bwd:
            _lib.check(_lib.lib.mvlpt_op_tpt_head_bwd(_ptr(w_d), scale, G, V, Cn, e, k, _ptr(dtxt.t), _ptr(ws.t), nb, _stream()), None,
                       "op_tpt_head_bwd")
    torch.cuda.synchronize()
    for b in (ws, loss, H, sel, dtxt) + ((z,) if z else ()):
        assert b.guards_intact()
    if not bwd:
        assert dtxt.untouched()
    return {"loss": loss.t.cpu(), "H": H.t.view(G, V).cpu(), "sel": sel.t.view(G, k).cpu(), "dtxt": dtxt.t.view(G * Cn, e).cpu(),
            "z": z.t.view(G, V, Cn).cpu() if z else None}


@functools.lru_cache(maxsize=None)
def reference(case, tie=False):
    """Computed once per case and shared; never modified."""
    G, V, Cn, e, k = case
    img, txt, w = R.tpt_inputs(*case, tie=tie)
    z, H, _, _, _, _ = R.tpt_forward(img, txt, R.TPT_SCALE, k)
    if tie:
        H = H.clone()
        H[:, 5] = H[:, 1]
    sel = R.select(H, k)
    loss, H2, _, dtxt, _ = R.tpt_ref(img, txt, R.TPT_SCALE, k, w, sel=sel)
    return img, txt, w, {"loss": loss, "H": H, "sel": sel, "dtxt": dtxt, "z": z}


def compare(got, ref, what=""):
    figs = {"H": R.rel_max1(got["H"], ref["H"]), "loss": R.rel_max1(got["loss"], ref["loss"]),
            "dtxt": R.rel(got["dtxt"], ref["dtxt"]) if float(ref["dtxt"].abs().max()) > 0 else float(got["dtxt"].abs().max())}
    if got["z"] is not None:
        figs["z"] = R.rel(got["z"], ref["z"])
    print(what, " ".join(f"{n} {v:.3e}" for n, v in figs.items()))
    assert torch.equal(got["sel"].long(), ref["sel"]), (got["sel"], ref["sel"])
    assert figs["H"] <= R.TPT_H_TOL and figs["loss"] <= R.TPT_LOSS_TOL and figs["dtxt"] <= R.TPT_DTXT_TOL
    assert figs.get("z", 0.0) <= R.TPT_Z_TOL


@pytest.mark.parametrize("case", R.TPT_CASES, ids=IDS)
def test_head_against_float64(case):
    G, V, Cn, e, k = case
    img, txt, w, ref = reference(case)
    got = call(img, txt, k, w, want_z=True)
    compare(got, ref, str(case))
    if Cn == 1:
        assert bool((got["loss"] == 0).all()) and bool((got["H"] == 0).all()) and bool((got["dtxt"] == 0).all())
    # without the optional output: the same bits
    again = call(img, txt, k, w, want_z=False)
    for n in ("loss", "H", "sel", "dtxt"):
        assert torch.equal(got[n], again[n]), n


def test_no_weights_are_weights_of_one():
    case = (2, 5, 7, 128, 2)
    img, txt, _, _ = reference(case)
    a, b = call(img, txt, 2, None), call(img, txt, 2, torch.ones(2))
    assert torch.equal(a["dtxt"], b["dtxt"])
    ref = R.tpt_ref(img, txt, R.TPT_SCALE, 2, None)
    assert R.rel(a["dtxt"], ref[3]) <= R.TPT_DTXT_TOL


@pytest.mark.parametrize("case", list(R.TPT_TIE_SEED_SHIFT), ids=[str(c) for c in R.TPT_TIE_SEED_SHIFT])
def test_identical_views_tie_exactly_and_the_lower_index_wins(case):
    G, V, Cn, e, k = case
    img, txt, w, ref = reference(case, True)
    got = call(img, txt, k, w)
    assert torch.equal(got["H"][:, 1], got["H"][:, 5])                   # bit-equal
    assert got["sel"][:, k - 1].tolist() == [1] * G and not bool((got["sel"] == 5).any())
    compare(got, ref, f"tie {case}")


def test_group_is_independent_of_the_batch():
    case = (3, 64, 17, 512, 6)
    img, txt, w, _ = reference(case)
    whole = call(img, txt, 6, w, want_z=True)
    for g in range(3):
        one = call(img[g:g + 1], txt[g * 17:(g + 1) * 17], 6, w[g:g + 1], want_z=True)
        assert torch.equal(one["loss"], whole["loss"][g:g + 1]) and torch.equal(one["H"], whole["H"][g:g + 1])
        assert torch.equal(one["sel"], whole["sel"][g:g + 1]) and torch.equal(one["z"], whole["z"][g:g + 1])
        assert torch.equal(one["dtxt"], whole["dtxt"][g * 17:(g + 1) * 17])


def test_view_position_does_not_change_its_entropy():
    case = (2, 64, 257, 576, 6)
    img, txt, _, _ = reference(case)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5))
    a, b = call(img, txt, 6, bwd=False), call(img[:, perm], txt, 6, bwd=False)
    assert torch.equal(a["H"][:, perm], b["H"])
    assert torch.equal(a["loss"], b["loss"]) or R.rel_max1(a["loss"], b["loss"]) <= R.TPT_LOSS_TOL     # the order of sel may differ


@pytest.mark.parametrize("case", [(4, 33, 65, 768, 3), (1, 128, 2191, 512, 12)], ids=str)
def test_two_calls_are_bit_equal(case):
    img, txt, w, _ = reference(case)
    a, b = call(img, txt, case[4], w, want_z=True), call(img, txt, case[4], w, want_z=True)
    for n in ("loss", "H", "sel", "dtxt", "z"):
        assert torch.equal(a[n], b[n]), n


def test_nan_view_goes_last():
    case = (2, 8, 9, 64, 8)
    img, txt, _, _ = reference(case)
    img = img.clone()
    img[0, 2, 3] = float("nan")
    got = call(img, txt, 8, bwd=False)
    assert int(got["sel"][0, 7]) == 2 and sorted(got["sel"][0].tolist()) == list(range(8))
    got = call(img, txt, 3, bwd=False)
    assert 2 not in got["sel"][0].tolist()


def test_refusals_return_err_arg_and_write_nothing():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream, tpt_workspace_bytes
    G, V, Cn, e, k = 2, 5, 7, 128, 2
    nb = tpt_workspace_bytes(G, V, Cn, e, k)
    img, txt = torch.randn(G, V, e, device=DEV), torch.randn(G * Cn, e, device=DEV)
    bufs = {"ws": Buf(nb // 4), "loss": Buf(G), "H": Buf(G * V), "sel": Buf(G * k, torch.int32), "z": Buf(G * V * Cn), "dtxt": Buf(G * Cn * e)}
    # the largest sizes any call below names still fit the buffers' elements or are refused before a launch
    bad = [dict(G=0), dict(G=_lib.TPT_MAX_GROUPS + 1), dict(V=0), dict(V=_lib.TPT_MAX_VIEWS + 1), dict(C=0), dict(C=_lib.TPT_MAX_CLASSES + 1),
           dict(e=0), dict(e=126), dict(e=1028), dict(k=0), dict(k=V + 1), dict(nb=nb - 1), dict(nb=0), dict(nb=-1), dict(ws=None)]
    out = C.c_int64(-5)
    for b in bad:
        a = dict(G=G, V=V, C=Cn, e=e, k=k, nb=nb, ws=bufs["ws"].t)
        a.update(b)
        with torch.cuda.device(DEV):
            rc = _lib.lib.mvlpt_op_tpt_head_fwd(_ptr(img), _ptr(txt), 100.0, a["G"], a["V"], a["C"], a["e"], a["k"], _ptr(bufs["loss"].t),
                                                _ptr(bufs["H"].t), _ptr(bufs["sel"].t), _ptr(bufs["z"].t), _ptr(a["ws"]), a["nb"], _stream())
            assert rc == _lib.ERR_ARG and _lib.last_error(None), b
            rc = _lib.lib.mvlpt_op_tpt_head_bwd(None, 100.0, a["G"], a["V"], a["C"], a["e"], a["k"], _ptr(bufs["dtxt"].t), _ptr(a["ws"]),
                                                a["nb"], _stream())
            assert rc == _lib.ERR_ARG and _lib.last_error(None), b
            if "nb" not in b and "ws" not in b:
                assert _lib.lib.mvlpt_tpt_workspace_bytes(a["G"], a["V"], a["C"], a["e"], a["k"], C.byref(out)) == _lib.ERR_ARG, b
                assert out.value == -5
    with torch.cuda.device(DEV):
        for miss in ("img", "txt", "loss", "H", "sel"):
            p = {"img": img, "txt": txt, "loss": bufs["loss"].t, "H": bufs["H"].t, "sel": bufs["sel"].t}
            p[miss] = None
            rc = _lib.lib.mvlpt_op_tpt_head_fwd(_ptr(p["img"]), _ptr(p["txt"]), 100.0, G, V, Cn, e, k, _ptr(p["loss"]), _ptr(p["H"]),
                                                _ptr(p["sel"]), None, _ptr(bufs["ws"].t), nb, _stream())
            assert rc == _lib.ERR_ARG, miss
        assert _lib.lib.mvlpt_op_tpt_head_bwd(None, 100.0, G, V, Cn, e, k, None, _ptr(bufs["ws"].t), nb, _stream()) == _lib.ERR_ARG
        assert _lib.lib.mvlpt_tpt_workspace_bytes(G, V, Cn, e, k, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for n, b in bufs.items():
        assert b.untouched(), n


def test_engine_binding_and_state_rule():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    eng = Engine(ARCHS["tiny"], device=torch.device(DEV))
    with pytest.raises(RuntimeError, match="tpt_head_bwd without tpt_head_fwd"):
        eng.tpt_head_bwd()
    case = (2, 5, 7, 128, 2)
    img, txt, w, ref = reference(case)
    loss, H, sel = eng.tpt_head_fwd(img.to(DEV), txt.to(DEV), R.TPT_SCALE, 2)
    dtxt = eng.tpt_head_bwd(w.to(DEV))
    ws_small = eng._tpt_ws
    compare({"loss": loss.cpu(), "H": H.cpu(), "sel": sel.cpu(), "dtxt": dtxt.cpu(), "z": None}, ref, "engine")
    out = eng.tpt_head_fwd(img.to(DEV), txt.to(DEV), R.TPT_SCALE, 2, want_logits=True)
    assert len(out) == 4 and R.rel(out[3], ref["z"]) <= R.TPT_Z_TOL and eng._tpt_ws is ws_small        # grow-only: reused
    with pytest.raises(RuntimeError):                                 # a refused forward leaves no state behind
        eng.tpt_head_fwd(img.to(DEV), txt.to(DEV), R.TPT_SCALE, 6)
    with pytest.raises(RuntimeError, match="tpt_head_bwd without tpt_head_fwd"):
        eng.tpt_head_bwd()
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        eng.tpt_head_fwd(img, txt.to(DEV), R.TPT_SCALE, 2)
    eng.close()
