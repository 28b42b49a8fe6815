"""Kernel-level tests of the deep-text-prompt glue (-m gpu; csrc/deep_text.hip through mvlpt_op_overwrite_ctx_rows and
mvlpt_op_gather_zero_ctx_grad).

overwrite_ctx_rows is data movement: bit-exact against an indexing expression, every other element still the sentinel.
gather_zero_ctx_grad sums C fp32 terms per output element: wave w adds its terms c = w, w + 16, ... in order (at most ceil(C / 16) - 1
roundings), then 15 roundings join the 16 partials, and the scale is a power of two.  Each rounding is at most 2^-24 of a partial sum,
which never exceeds S = sum_c |term|; the comparison with the float64 sum therefore allows
    (C + 15) * 2^-24 * S + 2^-24 * |out|
per element (the last term: the float64 reference is compared after the output's own rounding).  Two calls must agree bit for bit, and
with the bits of gather_ctx_grad, whose reduction order it shares.  The addressed rows must then be exactly zero in dx32 and in its 16-bit
copy in all three layouts (fp16 and bf16), every other byte, the unused tail of the mixed rows included, unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
SENTINEL = -12345.678
# (L, d, n_ctx): one float4 column / the test tower's rows / three column blocks of which the last is partial
GEOMETRIES = [(8, 4, 1), (77, 256, 4), (24, 516, 16)]


def _ctx_pos(C, L, n, g):
    """distinct, unsorted positions per class, never row 0"""
    return torch.stack([torch.randperm(L - 1, generator=g)[:n] + 1 for _ in range(C)]).int()


def _random16(shape, dtype, g):
    """16-bit tensor of random non-zero bytes (every byte in 1..254): a cleared byte cannot hide"""
    raw = torch.randint(1, 255, tuple(shape[:-1]) + (shape[-1] * 2,), generator=g, dtype=torch.uint8)
    return raw.view(dtype)


# ------------------------------------------------------------------------------------------------ overwrite
@pytest.mark.parametrize("C,L,d,n", [(1, 8, 4, 1), (5, 77, 256, 4), (37, 24, 516, 16)])
def test_overwrite_ctx_rows_bit_exact(C, L, d, n):
    from mvlpt_amd.engine import op_overwrite_ctx_rows
    g = torch.Generator().manual_seed(C * 100 + n)
    rows = torch.randn(n, d, generator=g)
    cp = _ctx_pos(C, L, n, g)
    want = torch.full((C, L, d), SENTINEL)
    want[torch.arange(C).view(C, 1), cp.long()] = rows
    for _ in range(2):
        x = torch.full((C, L, d), SENTINEL, device=DEV)
        got = op_overwrite_ctx_rows(rows.to(DEV), cp.to(DEV), x).cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    untouched = torch.ones(C, L, dtype=torch.bool)
    untouched[torch.arange(C).view(C, 1), cp.long()] = False
    assert bool((got[untouched] == torch.tensor(SENTINEL)).all()) and int(untouched.sum()) == C * (L - n)


def test_overwrite_ctx_rows_refuses_bad_arguments():
    from mvlpt_amd import _lib
    x = torch.zeros(2, 8, 8, device=DEV)
    rows, cp = torch.zeros(1, 8, device=DEV), torch.ones(2, 1, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()
    assert _lib.lib.mvlpt_op_overwrite_ctx_rows(P(rows), P(cp), P(x), 2, 8, 6, 1, None) == _lib.ERR_ARG      # d % 4
    assert _lib.lib.mvlpt_op_overwrite_ctx_rows(None, P(cp), P(x), 2, 8, 8, 1, None) == _lib.ERR_ARG
    assert _lib.lib.mvlpt_op_gather_zero_ctx_grad(_lib.DT_F16, P(x), None, 3, P(cp), 2, 8, 8, 1, P(rows), None, None) == _lib.ERR_ARG   # split16
    assert _lib.lib.mvlpt_op_gather_zero_ctx_grad(_lib.DT_F32, P(x), None, 0, P(cp), 2, 8, 8, 1, P(rows), None, None) == _lib.ERR_ARG   # dtype
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


def test_out_of_range_position_is_skipped():
    """An entry of ctx_pos outside [0, L) addresses no row: nothing is written or read for it."""
    from mvlpt_amd.engine import op_gather_zero_ctx_grad, op_overwrite_ctx_rows
    C, L, d = 3, 6, 8
    cp = torch.tensor([[1], [L], [-1]], dtype=torch.int32, device=DEV)
    x = torch.full((C, L, d), SENTINEL, device=DEV)
    rows = torch.ones(1, d, device=DEV)
    got = op_overwrite_ctx_rows(rows, cp, x).cpu()
    want = torch.full((C, L, d), SENTINEL)
    want[0, 1] = 1.0
    assert torch.equal(got, want)
    out = op_gather_zero_ctx_grad(x, None, cp).cpu()
    assert torch.equal(out, torch.ones(1, d))
    want[0, 1] = 0.0
    assert torch.equal(x.cpu(), want)


# ------------------------------------------------------------------------------------------------ gather and zero
@pytest.mark.parametrize("L,d,n", GEOMETRIES)
@pytest.mark.parametrize("C", [1, 15, 16, 17, 130])
def test_gather_zero_ctx_grad(C, L, d, n):
    from mvlpt_amd.engine import op_gather_ctx_grad, op_gather_zero_ctx_grad
    g = torch.Generator().manual_seed(C * 1000 + d + n)
    dx = torch.randn(C, L, d, generator=g)
    cp = _ctx_pos(C, L, n, g)
    idx = (torch.arange(C).view(C, 1), cp.long())
    picked = dx[idx].double()                                    # [C, n, d]
    scale_dev = torch.tensor([32.0, 1 / 32.0, 0.0, 0.0], device=DEV)
    exp32 = dx.clone()
    exp32[idx] = 0.0
    worst = 0.0
    # (split16, dtype of the 16-bit copy or None, scaled)
    variants = [(0, None, False)] + [(s, dt, (s + i) % 2 == 0) for s in (0, 1, 2) for i, dt in enumerate(DTYPES)]
    for split16, dt16, scaled in variants:
        inv = 1 / 32.0 if scaled else 1.0
        sc = scale_dev if scaled else None
        want = picked.sum(0) * inv
        S = picked.abs().sum(0) * inv
        pitch = d * (2 if split16 else 1)
        dx16 = _random16((C * L, pitch), dt16, g) if dt16 is not None else None
        plain = op_gather_ctx_grad(dx.to(DEV), cp.to(DEV), False, sc).cpu()
        outs = []
        for _ in range(2):
            a32 = dx.to(DEV)
            a16 = dx16.to(DEV) if dx16 is not None else None
            out = op_gather_zero_ctx_grad(a32, a16, cp.to(DEV), split16, sc, dtype=torch.bfloat16 if dt16 is None else None)
            outs.append((out.cpu(), a32.cpu(), None if a16 is None else a16.cpu()))
        out, a32, a16 = outs[0]
        assert torch.equal(out, outs[1][0]), "two calls are not bit-equal"
        assert torch.equal(out, plain), "not the bits of gather_ctx_grad's reduction"
        bound = (C + 15) * 2.0 ** -24 * S + 2.0 ** -24 * out.double().abs()
        excess = float(((out.double() - want).abs() - bound).max())
        worst = max(worst, float(((out.double() - want).abs() / bound.clamp_min(1e-300)).max()))
        assert excess <= 0.0, f"split16={split16} {dt16}: over the derived bound by {excess:.3e}"
        # the buffers afterwards
        assert torch.equal(a32.view(torch.int32), exp32.view(torch.int32)), "dx32: the addressed rows zero, every other element unchanged"
        if a16 is not None:
            exp16 = dx16.clone().view(torch.uint8).view(C, L, pitch * 2)
            # plain: d elements; pair: hi | lo, 2d elements; mixed pair: hi (2d bytes) | residual bytes (d), the tail stays
            live = 3 * d if split16 == 2 else pitch * 2
            sub = exp16[idx]
            sub[..., :live] = 0
            exp16[idx] = sub
            assert torch.equal(a16.view(torch.uint8).view(C, L, pitch * 2), exp16), f"dx16 after the call (split16={split16}, {dt16})"
            assert torch.equal(outs[1][2].view(torch.uint8), a16.view(torch.uint8))
    print(f"gather_zero_ctx_grad C={C} L={L} d={d} n={n}: worst |err| / bound {worst:.3f}")
