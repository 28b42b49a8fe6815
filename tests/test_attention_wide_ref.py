"""tests/attention_wide_ref.py without a GPU: the float64 restatement against torch's scaled_dot_product_attention, the two forms of
the reference against each other, and the teeth of the bound: four deliberately wrong references exceed it on the inputs of the GPU test."""
import pytest
import torch

from tests import attention_wide_ref as R

_CACHE = {}


def _case(c):
    """Inputs, reference and bound of one case, computed once."""
    w, L, H, N, _q, _lse, dtype = c
    key = (w, L, H, N, dtype)
    if key not in _CACHE:
        qkv = R.inputs(w, L, H, N, dtype)
        _CACHE[key] = (qkv, R.reference(qkv, N, L, H, w), R.reference_and_bound(qkv, N, L, H, w))
    return _CACHE[key]


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_restatement_is_scaled_dot_product_attention(c):
    w, L, H, N = c[:4]
    qkv, (out, lse), rb = _case(c)
    q, k, v = R.split_heads(qkv, N, L, H, w)
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v)          # float64, scale 1 / sqrt(w)
    assert (out - sdpa.permute(0, 2, 1, 3).reshape(N * L, H * w)).abs().max() < 1e-13
    # the bound's own reference (explicit maximum, sum, logarithm) is the same function
    assert (rb["out"][0] - out).abs().max() < 1e-13 and (rb["lse"][0] - lse).abs().max() < 1e-12
    for ref, bound in rb.values():
        assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all()) and ref.shape == bound.shape


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_bound_is_of_the_size_of_the_16_bit_roundings(c):
    """Not a blank cheque: relative to the largest |v| of its (sequence, head) the output bound stays below 8 u16 (P's rounding and the
    output's are 2 u16 at most; the rest is fp16's lost subnormal weights at L = 257) and the lse bound below 1e-3."""
    w, L, H, N, _q, _lse, dtype = c
    _qkv, (out, _), rb = _case(c)
    scale = R.split_heads(_qkv, N, L, H, w)[2].abs().amax((-1, -2))            # max |v| of the (sequence, head): what an output can reach
    b = rb["out"][1].view(N, L, H, w).permute(0, 2, 1, 3)
    assert float((b.amax((-1, -2)) / scale).max()) < 8 * R.U_OUT16[dtype]
    assert float(rb["lse"][1].max()) < 1e-3


# (one head has no neighbour: "next_head_v" runs on the cases with three)
MUTANTS = [(c, m) for m in ("scale8", "cols64", "key_L", "next_head_v") for c in R.CASES if not (m == "next_head_v" and c[2] == 1)]


@pytest.mark.parametrize("c,mutant", MUTANTS, ids=[f"{m}-{R.case_id(c)}" for c, m in MUTANTS])
def test_wrong_references_exceed_the_bound(c, mutant):
    w, L, H, N = c[:4]
    qkv, _ref, rb = _case(c)
    out, lse = R.reference(qkv, N, L, H, w, mutant)
    bad_out, ratio_out = R.violations(out, *rb["out"])
    bad_lse, ratio_lse = R.violations(lse, *rb["lse"])
    if L == 1 and mutant != "next_head_v":
        # one key: the output is v whatever the score; the lse carries the error
        assert bad_out == 0 and bad_lse > 0, (ratio_out, ratio_lse)
    else:
        assert bad_out > 0 and ratio_out > 10, (ratio_out, ratio_lse)
        if mutant != "next_head_v":
            assert bad_lse > 0, ratio_lse


def test_sequence_0_does_not_depend_on_the_batch():
    a, b = R.inputs(80, 65, 3, 1, R.F16), R.inputs(80, 65, 3, 2, R.F16)
    assert torch.equal(a, b[:65])


def test_computed_row_masks():
    assert R.computed_rows(2, 5, 0).all() and R.computed_rows(2, 5, 1).tolist() == [True] + [False] * 4 + [True] + [False] * 4
    assert R.computed_lse(1, 3, 2, 1).tolist() == [True, False, False, True, False, False]
