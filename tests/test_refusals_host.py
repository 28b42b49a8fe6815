"""CPU checks of the handle-less entries' refusals: one call per entry family that is turned down before any HIP call, with its return
code and the exact text mvlpt_last_error(NULL) then holds.  The pointers are never dereferenced (the refusal comes first), so
plain aligned numbers stand in for device memory."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096      # a non-null, 16-byte aligned "pointer"


@pytest.fixture(scope="module")
def L():
    if not os.path.isfile(os.path.join(ROOT, "mvlpt_amd", "libmvlpt_hip.so")):
        import __graft_entry__ as g
        g.build()
    from mvlpt_amd import _lib
    return _lib


def _optim_too_many_segs(L):
    hyper = L.MvlptOptimHyper(kind=L.OPTIM_SGD, lr=0.1, launch=1)
    return L.lib.mvlpt_op_optim_step(C.byref(hyper), P, P, None, None, 16, P, L.OPTIM_MAX_SEGS + 1, None, None, None)


# (id, call, return code, text)
CASES = [
    ("layernorm_fwd_ex-null", lambda L: L.lib.mvlpt_op_layernorm_fwd_ex(L.DT_F16, None, 1, P, P, P, 4, 64, 0, None),
     "ERR_ARG", "op_layernorm_fwd_ex: null pointer"),
    ("layernorm_fwd_ex-d6", lambda L: L.lib.mvlpt_op_layernorm_fwd_ex(L.DT_F16, P, 1, P, P, P, 4, 6, 0, None),
     "ERR_UNSUPPORTED", "op_layernorm_fwd_ex: d must be a multiple of 4 and at most 2048"),
    ("layernorm_bwd_ex-null", lambda L: L.lib.mvlpt_op_layernorm_bwd_ex(L.DT_F16, None, L.DT_F32, P, 1, P, None, P, P, 4, 64, 0, None),
     "ERR_ARG", "op_layernorm_bwd_ex: null pointer"),
    ("layernorm_bwd_ex-d6", lambda L: L.lib.mvlpt_op_layernorm_bwd_ex(L.DT_F16, P, L.DT_F32, P, 1, P, None, P, P, 4, 6, 0, None),
     "ERR_UNSUPPORTED", "op_layernorm_bwd_ex: d must be a multiple of 4 and at most 2048"),
    ("layernorm_fwd_split-f32", lambda L: L.lib.mvlpt_op_layernorm_fwd_split(L.DT_F32, P, P, P, P, 4, 64, None),
     "ERR_ARG", "layernorm_fwd_split: 16-bit output only"),
    ("cast_ex-format3", lambda L: L.lib.mvlpt_op_cast_ex(L.DT_F16, P, P, 4, 64, 3, None, None),
     "ERR_ARG", "op_cast_ex: dtype is fp16 or bf16, format in {0, 1, 2}, rows >= 0, d > 0"),
    ("pack_weight-short-ld", lambda L: L.lib.mvlpt_op_pack_weight(L.DT_F16, P, 8, 16, 0, 8, P, None),
     "ERR_ARG", "op_pack_weight: ld_out is shorter than a row of the output"),
    ("patchify-R-not-multiple", lambda L: L.lib.mvlpt_op_patchify(L.DT_F16, P, L.DT_F32, P, 1, 30, 8, 192, None),
     "ERR_UNSUPPORTED", "op_patchify: R must be a multiple of P"),
    ("nearest_workspace_bytes-k65", lambda L: L.lib.mvlpt_nearest_workspace_bytes(4, 100, 64, 65, None, C.byref(C.c_int64())),
     "ERR_UNSUPPORTED", "nearest_workspace_bytes: k exceeds MVLPT_NEAREST_MAX_K"),
    ("nearest_rows-null", lambda L: L.lib.mvlpt_op_nearest_rows(None, P, 4, 100, 64, 1, P, P, P, 0, None),
     "ERR_ARG", "op_nearest_rows: null argument"),
    ("eval_workspace_bytes-N0", lambda L: L.lib.mvlpt_eval_workspace_bytes(0, 5, None, C.byref(C.c_int64())),
     "ERR_ARG", "eval_workspace_bytes: N and C must be at least 1"),
    ("eval_count-ranges-without-n_pred_r",
     lambda L: L.lib.mvlpt_op_eval_count(P, 5, 2, 5, P, L.LABEL_INT64, 0, None, 0, P, P, P, 1, None, None, P, P, P, None, None, None, None),
     "ERR_ARG", "op_eval_count: task ranges need task, lo, hi, T >= 1, n_pred_r and n_hit_r together"),
    ("softmax_reg_workspace_bytes-K1", lambda L: L.lib.mvlpt_softmax_reg_workspace_bytes(10, 8, 1, C.byref(C.c_size_t())),
     "ERR_ARG", "softmax_reg_workspace_bytes: K must be at least 2"),
    ("softmax_reg_workspace_bytes-D6", lambda L: L.lib.mvlpt_softmax_reg_workspace_bytes(10, 6, 3, C.byref(C.c_size_t())),
     "ERR_ARG", "softmax_reg_workspace_bytes: D must be a multiple of 4, at least 4"),
    ("optim_step-too-many-segs", _optim_too_many_segs,
     "ERR_UNSUPPORTED", "op_optim_step: more than MVLPT_OPTIM_MAX_SEGS segments"),
    ("jpeg_idct-ragged-blocks", lambda L: L.lib.mvlpt_op_jpeg_idct(P, P, 10, 3, P, None),
     "ERR_ARG", "op_jpeg_idct: null / misaligned pointer, or n_blocks is not a positive multiple of blocks_w"),
]


@pytest.mark.parametrize("call,code,text", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal_code_and_text(L, call, code, text):
    rc = call(L)
    got = L.last_error(None)
    print(f"rc {rc}  last_error {got!r}")
    assert rc == getattr(L, code)
    assert got == text
