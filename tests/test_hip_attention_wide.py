"""mvlpt_op_attention_wide_fwd (-m gpu, kernel level): the attention forward for heads of 80 / 96 / 112 / 128 against the float64
reference of tests/attention_wide_ref.py under its derived per-element bound, `out` and `lse`; guard regions around and between the rows
the contract names; determinism; independence of a sequence from its batch; the refusals.

The destinations are views into larger buffers filled with a sentinel bit pattern: 4096 elements in front and behind, and (q_rows = 1)
the rows of every sequence that are not computed.  Worst error / bound over the cases below, as measured when the kernel was written:
DESIGN.md row m."""
import pytest
import torch

from tests import attention_wide_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
SENT16 = 0x7B7B          # fp16 60256.0 / bf16 3.26e36: no attention output of these inputs
SENT32 = -7.0e37

_REF = {}


def _ref(c):
    w, L, H, N, _q, _lse, dtype = c
    key = (w, L, H, N, dtype)
    if key not in _REF:
        qkv = R.inputs(w, L, H, N, dtype)
        _REF[key] = (qkv, R.reference_and_bound(qkv, N, L, H, w))
    return _REF[key]


def _guarded(n, dtype):
    """(buffer, view of n elements behind GUARD sentinels, with GUARD more behind it)"""
    if dtype == torch.float32:
        buf = torch.full((n + 2 * GUARD,), SENT32, device=DEV, dtype=torch.float32)
    else:
        buf = torch.full((n + 2 * GUARD,), SENT16, device=DEV, dtype=torch.int16).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def _is_sentinel(t):
    return (t == SENT32) if t.dtype == torch.float32 else (t.view(torch.int16) == SENT16)


def _run(c, qkv_dev=None):
    from mvlpt_amd import engine as E
    w, L, H, N, q_rows, want_lse, dtype = c
    qkv = _ref(c)[0].to(DEV) if qkv_dev is None else qkv_dev
    obuf, out = _guarded(N * L * H * w, dtype)
    lbuf, lse = _guarded(N * H * L, torch.float32)
    E.op_attention_wide_fwd(qkv, N, L, H, w, q_rows=q_rows, want_lse=want_lse, out=out.view(N * L, H * w), lse=lse if want_lse else None)
    torch.cuda.synchronize()
    return obuf.cpu(), out.view(N * L, H * w).cpu(), lbuf.cpu(), lse.cpu()


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_against_float64_under_the_derived_bound(c):
    w, L, H, N, q_rows, want_lse, dtype = c
    _qkv, rb = _ref(c)
    obuf, out, lbuf, lse = _run(c)
    rows, lrows = R.computed_rows(N, L, q_rows), R.computed_lse(N, L, H, q_rows)
    # every sentinel survives: the guards, and the rows the contract does not name
    assert bool(_is_sentinel(obuf[:GUARD]).all()) and bool(_is_sentinel(obuf[-GUARD:]).all()), "out: a guard region was written"
    assert bool(_is_sentinel(out[~rows]).all()), "out: a row beyond q_rows was written"
    assert bool(_is_sentinel(lbuf[:GUARD]).all()) and bool(_is_sentinel(lbuf[-GUARD:]).all()), "lse: a guard region was written"
    if want_lse:
        assert bool(_is_sentinel(lse[~lrows]).all()), "lse: an entry beyond q_rows was written"
    else:
        assert bool(_is_sentinel(lse).all()), "lse: written although the pointer was null"
    ref, bound = rb["out"]
    bad, ratio = R.violations(out[rows].double(), ref[rows], bound[rows])
    print(f"{R.case_id(c)}: out worst error / bound {ratio:.3f}")
    assert bad == 0, f"out: {bad} elements outside the bound, worst error / bound {ratio:.3f}"
    if want_lse:
        ref, bound = rb["lse"]
        bad, ratio = R.violations(lse[lrows].double(), ref[lrows], bound[lrows])
        print(f"{R.case_id(c)}: lse worst error / bound {ratio:.3f}")
        assert bad == 0, f"lse: {bad} entries outside the bound, worst error / bound {ratio:.3f}"


@pytest.mark.parametrize("c", [R.CASES[5], R.CASES[9], R.CASES[13], R.CASES[16]], ids=R.case_id)
def test_two_calls_are_bit_equal(c):
    a, b = _run(c), _run(c)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("w,L,H,dtype", [(80, 65, 3, R.F16), (80, 257, 3, R.BF16), (112, 130, 1, R.F16), (128, 257, 1, R.BF16)])
def test_sequence_0_does_not_depend_on_the_batch(w, L, H, dtype):
    one = _run((w, L, H, 1, 0, True, dtype), R.inputs(w, L, H, 1, dtype).to(DEV))
    two = _run((w, L, H, 2, 0, True, dtype), R.inputs(w, L, H, 2, dtype).to(DEV))
    assert torch.equal(one[1].view(torch.int16), two[1][:L].view(torch.int16))
    lse1, lse2 = one[3].view(1, H, L), two[3].view(2, H, L)
    assert torch.equal(lse1[0], lse2[0])


def test_refusals_launch_nothing():
    """A width outside the list: MVLPT_ERR_UNSUPPORTED; a null pointer, a non-positive size, an fp32 dtype: MVLPT_ERR_ARG.  (The entry
    has no `causal` argument: the kernel is non-causal, and launch_attn_fwd_wide answers a causal request with hipErrorInvalidValue.)
    Nothing is written in either case."""
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    lib = _lib.lib
    N, L, H = 1, 15, 1
    for w in (64, 72, 88, 104, 144, 0, -80):
        ww = max(abs(w), 16)
        qkv = torch.zeros(N * L, 3 * H * ww, device=DEV, dtype=torch.float16)
        obuf, out = _guarded(N * L * H * ww, torch.float16)
        rc = lib.mvlpt_op_attention_wide_fwd(_lib.DT_F16, _ptr(qkv), _ptr(out), None, N, L, H, w, 0, _stream())
        assert rc == _lib.ERR_UNSUPPORTED and "80, 96, 112 or 128" in _lib.last_error(None), w
        torch.cuda.synchronize()
        assert bool(_is_sentinel(obuf).all())
    qkv = torch.zeros(N * L, 3 * H * 80, device=DEV, dtype=torch.float16)
    obuf, out = _guarded(N * L * H * 80, torch.float16)
    bad = [(_lib.DT_F16, None, _ptr(out), N, L, H, 0), (_lib.DT_F16, _ptr(qkv), None, N, L, H, 0), (_lib.DT_F16, _ptr(qkv), _ptr(out), 0, L, H, 0),
           (_lib.DT_F16, _ptr(qkv), _ptr(out), N, 0, H, 0), (_lib.DT_F16, _ptr(qkv), _ptr(out), N, L, 0, 0),
           (_lib.DT_F16, _ptr(qkv), _ptr(out), N, L, H, -1), (_lib.DT_F32, _ptr(qkv), _ptr(out), N, L, H, 0)]
    for dt, q, o, n, l, h, qr in bad:
        assert lib.mvlpt_op_attention_wide_fwd(dt, q, o, None, n, l, h, 80, qr, _stream()) == _lib.ERR_ARG, (dt, n, l, h, qr)
    torch.cuda.synchronize()
    assert bool(_is_sentinel(obuf).all())
