"""Kernel-level tests of the fp32 glue around the towers (-m gpu): the gradient scale (one-workgroup and two-stage path), the prompt-row
and context-gradient reductions, the CLS-only attention backward, and the data-movement kernels at the towers' entries (copy_rows,
overwrite_rows, assemble_tokens, assemble_prompts + build_ctx_pos + eot_rows).  References: tests/head_ref.py (float64, checked on the CPU
by tests/test_head_ref.py) or plain indexing expressions, which must match bit for bit.  Every kernel runs twice: bit-identical."""
import pytest
import torch

from tests import head_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.element_size() == 4 else t.contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------------ gradient scale
GS_N = [1, 3, 4, 5, 4095, 4097, 2 ** 17 - 1, 2 ** 17, 2 ** 17 + 1, 3 * 10 ** 6]


def _grad_scale_both_paths(v):
    """scale_dev of `v` from a 16-byte aligned copy (one workgroup up to n = 2^17) and from a copy 4 bytes into an allocation (always
    the two-stage path), each run twice."""
    from mvlpt_amd.engine import op_grad_scale
    n = v.numel()
    aligned = v.to(DEV)
    buf = torch.zeros(n + 1, device=DEV)
    buf[1:] = aligned
    shifted = buf[1:]
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    out = {}
    for name, t in (("aligned", aligned), ("shifted", shifted)):
        for target in (64.0, 128.0):
            a, b = op_grad_scale(t, target).cpu(), op_grad_scale(t, target).cpu()
            assert torch.equal(_bits(a), _bits(b)), f"{name}: not bit-stable"
            out[name, target] = a
    return out


def _check_grad_scale(v, what):
    got = _grad_scale_both_paths(v)
    for target in (64.0, 128.0):
        want = torch.tensor(R.scale_rule(v.numpy(), target), dtype=torch.float32)
        for name in ("aligned", "shifted"):
            sc = got[name, target]
            print(f"grad_scale n={v.numel()} {what} target={target:.0f} {name}: {sc.tolist()} want {want.tolist()}")
            assert torch.equal(_bits(sc[:2]), _bits(want)), f"{what} {name} target {target}: {sc.tolist()} != {want.tolist()}"
        assert torch.equal(_bits(got["aligned", target]), _bits(got["shifted", target])), f"{what}: the two paths disagree"
    return got


@pytest.mark.parametrize("n", GS_N)
def test_grad_scale_is_the_power_of_two_rule(n):
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g) * 0.01
    tail = n - 1 if n % 4 == 0 else n - (n % 4)                  # first element the float4 loop does not cover
    for what, idx in (("max at 0", 0), ("max at n-1", n - 1), ("max in the tail", tail), ("max inside", n // 2)):
        v = base.clone()
        v[idx] = -3.7 if idx % 2 else 5.3
        got = _check_grad_scale(v, what)
        assert float(got["aligned", 64.0][2]) == float(v.abs().max())


@pytest.mark.parametrize("n", [1, 5, 4097, 2 ** 17 + 1])
def test_grad_scale_edge_values(n):
    g = torch.Generator().manual_seed(n + 1)
    base = torch.randn(n, generator=g) * 0.01
    _check_grad_scale(torch.zeros(n), "all zeros")                               # -> 1
    neg0 = torch.zeros(n)
    neg0[n // 2] = -0.0
    _check_grad_scale(neg0, "zeros and -0.0")                                    # -> 1
    for idx in sorted({0, n // 2, n - 1}):
        v = base.clone()
        v[idx] = float("inf") if idx % 2 else float("-inf")
        _check_grad_scale(v, f"one inf at {idx}")                                # -> 1
        v = base.clone()
        v[idx] = float("nan")
        _check_grad_scale(v, f"one NaN at {idx}")                                # -> 1
    tiny = torch.zeros(n)
    tiny[n - 1] = 1e-40                                                          # a denormal amax: k = 7 + 132 -> clamped to 60
    assert 0 < float(tiny[n - 1]) < 1.2e-38
    _check_grad_scale(tiny, "denormal amax")
    tiny[0] = -3e-30                                                             # small but normal: k = 7 + 97 -> 60
    _check_grad_scale(tiny, "1e-30 amax")
    huge = base.clone()
    huge[n // 2] = -3e38                                                         # k = 7 - 128 -> clamped to -60
    _check_grad_scale(huge, "3e38 amax")


# ------------------------------------------------------------------------------------------------ reductions over the batch / the classes
RED_SIZES = [1, 5, 16, 17, 100, 256]
RED_D = [128, 192, 768, 1024]


def _random16(shape, dtype, g):
    """16-bit tensor of random non-zero bytes (every byte in 1..254): a cleared byte cannot hide."""
    raw = torch.randint(1, 255, tuple(shape[:-1]) + (shape[-1] * 2,), generator=g, dtype=torch.uint8)
    return raw.view(dtype)


@pytest.mark.parametrize("d", RED_D)
@pytest.mark.parametrize("B", RED_SIZES)
def test_reduce_prompt_rows(B, d):
    """REDUCE_TOL = 1e-6 * max|ref| is the bound of test_grouped_ctx_grad_gather_deterministic_and_exact; a plain fp32 host sum of 256
    rows stays inside it (tests/test_head_ref.py), so B = 256 keeps it.  zero_after must clear exactly the reduced rows of dx32 and of
    its 16-bit copy in each of the three layouts, and touch no other byte."""
    from mvlpt_amd.engine import op_reduce_prompt_rows
    row0 = 1
    scale_dev = torch.tensor([32.0, 1 / 32.0, 0.0], device=DEV)
    # (zero_after, split16, dtype of the 16-bit copy or None, scale, vmask)
    variants = [(False, 0, None, False, False), (False, 0, torch.float16, True, True)]
    variants += [(True, s, dt, (s + i) % 2 == 0, (s + i) % 2 == 1) for s in (0, 1, 2) for i, dt in enumerate(DTYPES)]
    for n in (1, 4, 16):
        L = row0 + n + 2
        g = torch.Generator().manual_seed(B * 1000 + d + n)
        dx = torch.randn(B, L, d, generator=g)
        vmask = (torch.rand(B, n, d, generator=g) > 0.25).float() / 0.75
        for zero_after, split16, dt16, use_scale, use_mask in variants:
            pitch = d * (2 if split16 else 1)
            dx16 = _random16((B * L, pitch), dt16, g) if dt16 is not None else None
            rows = dx[:, row0:row0 + n]
            want = (rows * vmask if use_mask else rows).double().sum(0) * (1 / 32.0 if use_scale else 1.0)
            outs = []
            for _ in range(2):
                a32 = dx.to(DEV)
                a16 = dx16.to(DEV) if dx16 is not None else None
                out = op_reduce_prompt_rows(a32, a16, row0, n, scale_dev if use_scale else None, zero_after, split16,
                                            vmask.to(DEV) if use_mask else None)
                outs.append((out.cpu(), a32.cpu(), None if a16 is None else a16.cpu()))
            assert torch.equal(outs[0][0], outs[1][0]), "not bit-stable from run to run"
            out, a32, a16 = outs[0]
            err = R.rel(out, want)
            assert err <= R.REDUCE_TOL, f"n={n} zero_after={zero_after} split16={split16} {dt16}: {err:.3e}"
            # the buffers afterwards: reduced rows all-zero bits (when asked), every other byte as before
            exp32 = dx.clone()
            if zero_after:
                exp32[:, row0:row0 + n] = 0.0
            assert torch.equal(_bits(a32), _bits(exp32)), f"dx32 after the call (zero_after={zero_after})"
            if a16 is not None:
                exp16 = dx16.clone().view(torch.uint8).view(B, L, pitch * 2)
                if zero_after:
                    # plain: d elements; pair: hi | lo, 2d elements; mixed pair: hi (2d bytes) | residual bytes (d): the rest is unused
                    exp16[:, row0:row0 + n, :(3 * d if split16 == 2 else pitch * 2)] = 0
                assert torch.equal(a16.view(torch.uint8).view(B, L, pitch * 2), exp16), \
                    f"dx16 after the call (zero_after={zero_after}, split16={split16}, {dt16})"
        print(f"reduce_prompt_rows B={B} d={d} n={n}: last err {err:.2e}")


@pytest.mark.parametrize("d", RED_D)
@pytest.mark.parametrize("C", RED_SIZES)
def test_gather_ctx_grad(C, d):
    """Generic context: the sum over the classes, REDUCE_TOL as above.  Per class: a copy times a power of two, bit-exact."""
    from mvlpt_amd.engine import op_gather_ctx_grad
    scale_dev = torch.tensor([64.0, 1 / 64.0, 0.0], device=DEV)
    for n in (1, 4, 16):
        L = n + 6
        g = torch.Generator().manual_seed(C * 1000 + d + n)
        dx = torch.randn(C, L, d, generator=g)
        ctx_pos = torch.stack([torch.randperm(L - 1, generator=g)[:n] + 1 for _ in range(C)]).int()      # distinct, unsorted, per class
        picked = dx[torch.arange(C).view(C, 1), ctx_pos.long()]                                            # [C, n, d]
        for sc, inv in ((None, 1.0), (scale_dev, 1 / 64.0)):
            a = op_gather_ctx_grad(dx.to(DEV), ctx_pos.to(DEV), False, sc).cpu()
            b = op_gather_ctx_grad(dx.to(DEV), ctx_pos.to(DEV), False, sc).cpu()
            assert torch.equal(a, b) and a.shape == (n, d)
            err = R.rel(a, picked.double().sum(0) * inv)
            assert err <= R.REDUCE_TOL, f"generic n={n}: {err:.3e}"
            p = op_gather_ctx_grad(dx.to(DEV), ctx_pos.to(DEV), True, sc).cpu()
            q = op_gather_ctx_grad(dx.to(DEV), ctx_pos.to(DEV), True, sc).cpu()
            assert torch.equal(p, q) and torch.equal(p, picked * inv), f"per class n={n}"
        print(f"gather_ctx_grad C={C} d={d} n={n}: generic err {err:.2e}")


# ------------------------------------------------------------------------------------------------ attention backward, CLS query only
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", [(1, 1), (3, 2), (7, 12)])
@pytest.mark.parametrize("L", [1, 5, 16, 50, 63, 64, 65, 197, 205, 256, 577])
def test_attention_bwd_cls(L, N, H, dtype):
    """ATTN_TOL = TOL[dtype] * 3 per third of dqkv is the bound of test_attention_fwd_bwd.  lse and O come from the float64 forward of
    the rounded inputs; dqkv is pre-filled with NaN (every element must be written) and the lse of the queries > 0 is NaN (never read).

    At L = 1 the softmax over the single key is 1 and O = v_0, so the float64 dQ_0 and dK_0 are exactly 0: the kernel has to return
    exact zeros there, which it does because delta = dO.O and dp = dO.v are summed through the same chain."""
    from mvlpt_amd.engine import op_attention_bwd_cls
    d = H * 64
    qkv, do, lse, o_cls = R.attn_cls_inputs(N, L, H, dtype)
    want = R.attn_bwd_cls_ref(qkv, o_cls, do, lse, N, L, H)
    a = op_attention_bwd_cls(qkv.to(DEV), o_cls.to(DEV), do.to(DEV), lse.to(DEV), N, L, H).cpu()
    b = op_attention_bwd_cls(qkv.to(DEV), o_cls.to(DEV), do.to(DEV), lse.to(DEV), N, L, H, fill=1.0).cpu()
    assert bool(torch.isfinite(a.float()).all()), "an element of dqkv was not written"
    assert torch.equal(_bits(a), _bits(b)), "not bit-stable (or an element kept its pre-filled value)"
    assert bool((a.view(N, L, 3 * d)[:, 1:, :d] == 0).all()), "dQ of a query > 0 is not zero"
    errs = []
    for i, nm in enumerate("qkv"):
        ref = want[:, i * d:(i + 1) * d]
        e = R.rel(a[:, i * d:(i + 1) * d], ref)
        errs.append(e)
        print(f"  d{nm}: max|got - ref| {float((a[:, i * d:(i + 1) * d].double() - ref).abs().max()):.3e}, max|ref| {float(ref.abs().max()):.3e}")
        assert e <= R.ATTN_TOL[dtype], f"d{nm}: {e:.3e}"
    print(f"attention_bwd_cls L={L} N={N} H={H} {dtype}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e}")


# ------------------------------------------------------------------------------------------------ data movement
@pytest.mark.parametrize("rows,n_src,width,dtype", [(1, 1, 4, torch.float32), (7, 5, 192, torch.float32), (77, 200, 136, torch.float16),
                                                    (300, 64, 16, torch.uint8), (3000, 700, 1024, torch.float32)])
def test_copy_rows_gather_and_scatter_bit_exact(rows, n_src, width, dtype):
    """The last case has more 16-byte chunks than the grid has threads: every thread loops."""
    from mvlpt_amd.engine import op_copy_rows
    g = torch.Generator().manual_seed(rows + width)
    nbytes = width * torch.empty(0, dtype=dtype).element_size()
    src = torch.randint(0, 256, (n_src, nbytes), generator=g, dtype=torch.uint8).view(dtype)
    idx = torch.randint(0, n_src, (rows,), generator=g)                      # gather: repeats allowed
    a, b = op_copy_rows(src.to(DEV), idx.to(DEV)).cpu(), op_copy_rows(src.to(DEV), idx.to(DEV)).cpu()
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(src[idx]))
    # scatter through a permutation: rows of `src2` land on distinct rows of a larger destination, the others stay as they were
    n_dst = rows + 5
    perm = torch.randperm(n_dst, generator=g)[:rows]
    src2 = torch.randint(0, 256, (rows, nbytes), generator=g, dtype=torch.uint8).view(dtype)
    dst0 = torch.randint(0, 256, (n_dst, nbytes), generator=g, dtype=torch.uint8).view(dtype)
    want = dst0.clone()
    want[perm] = src2
    got = [op_copy_rows(src2.to(DEV), perm.to(DEV), dst=dst0.to(DEV)).cpu() for _ in range(2)]
    assert torch.equal(_bits(got[0]), _bits(got[1])) and torch.equal(_bits(got[0]), _bits(want))
    untouched = torch.ones(n_dst, dtype=torch.bool)
    untouched[perm] = False
    assert int(untouched.sum()) == 5 and torch.equal(_bits(got[0][untouched]), _bits(dst0[untouched]))


def test_copy_rows_refuses_rows_that_are_not_16_byte_multiples():
    from mvlpt_amd.engine import op_copy_rows
    with pytest.raises(RuntimeError):
        op_copy_rows(torch.zeros(4, 3, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("B,L,d,n", [(1, 2, 128, 1), (5, 9, 192, 5), (33, 7, 128, 1), (300, 20, 1024, 16)])
@pytest.mark.parametrize("masked", [False, True])
def test_overwrite_rows_bit_exact(B, L, d, n, masked):
    from mvlpt_amd.engine import op_overwrite_rows
    g = torch.Generator().manual_seed(B + L + d + n)
    x0, rows = torch.randn(B, L, d, generator=g), torch.randn(n, d, generator=g)
    vmask = (torch.rand(B, n, d, generator=g) > 0.3).float() / 0.7 if masked else None
    want = x0.clone()
    want[:, 1:1 + n] = rows * vmask if masked else rows
    got = [op_overwrite_rows(rows.to(DEV), x0.to(DEV), vmask.to(DEV) if masked else None).cpu() for _ in range(2)]
    assert torch.equal(_bits(got[0]), _bits(got[1])) and torch.equal(_bits(got[0]), _bits(want))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n_vpt", [0, 1, 5])
@pytest.mark.parametrize("B,G2,d", [(1, 1, 128), (3, 4, 192), (5, 49, 768), (2, 9, 1024), (3, 5, 1280), (45, 196, 768)])
def test_assemble_tokens(B, G2, d, n_vpt, masked):
    """LayerNorm rows against float64 at LN_TOL = 1e-5 (test_layernorm_fwd_bwd's fp32 bound), prompt rows (times their dropout mask)
    bit-exact.  (45, 196, 768) has more rows than the grid has waves: every wave loops and prefetches its next row."""
    from mvlpt_amd.engine import op_assemble_tokens
    if masked and n_vpt == 0:
        with pytest.raises(RuntimeError):           # a dropout mask without prompt rows is refused
            op_assemble_tokens(torch.zeros(B * G2, d, device=DEV), torch.zeros(d, device=DEV), torch.zeros(1 + G2, d, device=DEV),
                               torch.ones(d, device=DEV), torch.zeros(d, device=DEV), B, None, torch.ones(B, 1, d, device=DEV))
        return
    g = torch.Generator().manual_seed(B * 100 + G2 + d + n_vpt)
    pe, cls, pos = torch.randn(B * G2, d, generator=g) * 2, torch.randn(d, generator=g), torch.randn(1 + G2, d, generator=g) * 0.5
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    vpt = torch.randn(n_vpt, d, generator=g) if n_vpt else None
    vmask = (torch.rand(B, n_vpt, d, generator=g) > 0.3).float() / 0.7 if masked else None
    want, is_prompt = R.assemble_tokens_ref(pe, cls, pos, gamma, beta, B, vpt, vmask)
    dev = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    got = [op_assemble_tokens(dev(pe), dev(cls), dev(pos), dev(gamma), dev(beta), B, dev(vpt), dev(vmask)).cpu() for _ in range(2)]
    assert torch.equal(_bits(got[0]), _bits(got[1]))
    x = got[0]
    assert x.shape == want.shape and bool(torch.isfinite(x).all()), "a row was not written"
    err = R.rel(x[:, ~is_prompt], want[:, ~is_prompt])
    print(f"assemble_tokens B={B} G2={G2} d={d} n_vpt={n_vpt} masked={masked}: LayerNorm rows {err:.2e}")
    assert err <= R.LN_TOL
    if n_vpt:
        assert torch.equal(_bits(x[:, is_prompt]), _bits(want[:, is_prompt].float()))


@pytest.mark.parametrize("C,L,d", [(1, 12, 128), (7, 40, 192), (37, 77, 128), (300, 77, 512)])
@pytest.mark.parametrize("mode", ["generic-end", "generic-middle", "generic-front", "per-class-end", "per-class-middle", "no-ctx"])
def test_assemble_prompts_bit_exact(C, L, d, mode):
    """x, the context positions and the EOT rows of the text tower's entry against indexing expressions (the style of
    test_grouped_assembly_bit_exact).  (300, 77, 512) makes every thread of the capped grid loop."""
    from mvlpt_amd.engine import op_assemble_prompts
    from mvlpt_amd.model import build_prompt_layout
    g = torch.Generator().manual_seed(C + L + d + len(mode))
    n = 0 if mode == "no-ctx" else 5
    per_class = mode.startswith("per-class")
    name_lens = [1 + int(v) for v in torch.randint(0, 4, (C,), generator=g)]
    layout = build_prompt_layout(name_lens, n, L, mode.split("-")[-1] if n else "end")
    prefix, suffix = torch.randn(C, 1, d, generator=g), torch.randn(C, L - 1 - n, d, generator=g)
    ctx = None if n == 0 else torch.randn(*((C, n, d) if per_class else (n, d)), generator=g)
    pos = torch.randn(L + 3, d, generator=g)
    eot = torch.randint(1, L, (C,), generator=g, dtype=torch.int32)
    dev = lambda t: None if t is None else t.to(DEV)   # noqa: E731
    runs = [op_assemble_prompts(dev(prefix), dev(suffix), dev(ctx), dev(layout), dev(pos), dev(eot)) for _ in range(2)]
    x, ctx_pos, rows = runs[0]
    assert torch.equal(_bits(x), _bits(runs[1][0])) and torch.equal(rows, runs[1][2])
    fixed = torch.cat([prefix, suffix], dim=1)                                             # [C, L - n, d]
    if n:
        cls_ctx = ctx if per_class else ctx.unsqueeze(0).expand(C, n, d)
        table = torch.cat([fixed, cls_ctx], dim=1)                                         # [C, L, d]
    else:
        table = fixed
    idx = torch.where(layout >= 0, layout, (L - n) + (-layout - 1)).long()                 # row of `table` per position
    want = torch.gather(table, 1, idx.view(C, L, 1).expand(C, L, d)) + pos[:L]
    assert torch.equal(_bits(x.cpu()), _bits(want))
    assert torch.equal(rows.cpu(), (torch.arange(C) * L).int() + eot)
    if n:
        assert torch.equal(ctx_pos, runs[1][1])
        want_pos = torch.zeros(C, n, dtype=torch.int32)
        for c in range(C):
            for i in range(L):
                if layout[c, i] < 0:
                    want_pos[c, -int(layout[c, i]) - 1] = i
        assert torch.equal(ctx_pos.cpu(), want_pos)
    else:
        assert ctx_pos is None
