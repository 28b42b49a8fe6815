"""The MFMA GEMMs at kernel level (-m gpu), across every route of gemm.hip's launch_one, every epilogue and every operand format, against
the float64 references and per-element bounds of tests/gemm_ref.py.

Every case (1) asserts the kernel it reaches through mvlpt_op_gemm_route, so a moved routing threshold fails here instead of silently
moving the coverage, (2) checks the project's existing max-norm bound of that epilogue and format, (3) checks the per-element bound with no
element exempt, (4) runs a second time and compares bit for bit; epilogue 2 additionally runs in place (out aliases resid), which is how the
towers use it; epilogue 4 runs again with A at a padded pitch (NaN padding) and epilogue 7 with a padded output (sentinel padding), both
bit-identical to the dense call, so every kernel's own loader sees lda; pair and mixed operands also write the other pair format on 5 / 6.  Most of the matrix runs on a 32-CU partition stream: the routing thresholds scale with the stream's compute units, so
shapes of a few thousand rows reach every kernel with several ragged rounds (and the partitioned launch path is tested at kernel level).

The references are float64 matmuls on the device; every case checks the last rows of that product against a float64 matmul on the host.

Cells the launcher cannot reach: gemm_bt_phased_kernel with a mixed pair (it has no fp8 stages: launch_one keeps a_split == 2 off it) and
with K_eff < 2048 (so K in {64, 128, 192} does not exist there); gemm_pc_kernel with a single operand; the 4-deep 128x128 ring and the
3-deep 256x128 ring of gemm_bt_kernel with anything but a folded consumer (epilogues 0 / 1 / 5 / 7 through mvlpt_op_gemm_folded, which
has no pitch arguments: those two rings are instantiations of the same gemm_bt_kernel source whose loader the 256x256 and 128x128
two-per-CU cases run with a padded A).  Not covered: a single operand writing a mixed pair (out_lo8 with a_split == 0; no tower does).
"""
import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}
NAN16 = {torch.float16: 0x7e01, torch.bfloat16: 0x7fc1}       # a NaN of the 16-bit type (its bytes are NaNs of both fp8 types too)
SENTINEL = 0x5a5a


def _E():
    from mvlpt_amd import engine
    return engine


def _L():
    from mvlpt_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def stream32(dev):
    return _E().partition_stream(dev, 0, 32)


def _family(name):
    L = _L()
    return {"pcp": L.GEMM_PCP, "big_multi": L.GEMM_BT_256x256_R2, "big_one": L.GEMM_BT_256x256_R2, "small": L.GEMM_BT_128x128_R2,
            "pc": L.GEMM_PC, "phased": L.GEMM_PHASED, "r4": L.GEMM_BT_128x128_R4, "r3": L.GEMM_BT_256x128_R3}[name]


GEOMETRY = {"pcp": (256, 128, 3), "big_multi": (256, 256, 2), "big_one": (256, 256, 2), "small": (128, 128, 2), "pc": (128, 128, 4),
            "phased": (256, 128, 3), "r4": (128, 128, 4), "r3": (256, 128, 3)}


def _launch(pr, t, epi, out2, out_lo8, dev, A=None, lda=0, ldo=0, out=None, resid=None):
    """One launch through mvlpt_op_gemm_ex on device operands `t`; -> (out, out2 or None).  Pair outputs start from zeros so that the
    slots a mixed pair leaves unused compare equal."""
    E = _E()
    M, N = pr.M, pr.N
    if out is None:
        if epi in (R.EPI_RESID32, R.EPI_STORE32):
            out = torch.empty(M, N, device=dev, dtype=torch.float32)
        elif epi in (R.EPI_GELU_SPLIT, R.EPI_GELUBWD_SPLIT, R.EPI_STORE_SPLIT):
            out = torch.zeros(M, 2 * N, device=dev, dtype=pr.dtype)
        else:
            out = torch.empty(M, N, device=dev, dtype=pr.dtype)
    o2 = torch.empty(M, N, device=dev, dtype=pr.dtype) if out2 else None
    grad = epi in (R.EPI_GELUBWD, R.EPI_GELUBWD_SPLIT)
    E.op_gemm_ex(t["A"] if A is None else A, t["Bt"], epi, M, N, pr.K, out, bias=None if grad else t["bias"], aux=t["aux"] if grad else None,
                 resid=(t["resid"] if resid is None else resid) if epi == R.EPI_RESID32 else None, out2=o2, a_split=R.A_SPLIT[pr.fmt], lda=lda,
                 ldo=ldo, ldb=pr.ldb, w8_exp=pr.w8_exp, out_lo8=out_lo8)
    return out, o2


def _padded_a(pr, dev):
    """A at a row pitch 64 elements wider, the padding (and the unused quarter of a mixed row) filled with NaNs."""
    wide = R.with_pitch(pr.A, pr.A.shape[1] + 64, NAN16[pr.dtype])
    if pr.fmt == "mixed":
        wide.view(torch.int16)[:, pr.K + pr.K // 2:2 * pr.K] = NAN16[pr.dtype]
    return wide.to(dev)


def _device_operands(pr, dev):
    return {k: getattr(pr, k).to(dev) for k in ("A", "Bt", "bias", "resid", "aux")}


def _products(pr, dev, host_rows=128):
    """Float64 product and magnitude sum on the device, the last rows checked against the host's float64 matmul."""
    acc, S = pr.products(dev)
    rows = slice(max(0, pr.M - host_rows), pr.M)
    h_acc, h_S = pr.products("cpu", rows)
    assert float((acc[rows].cpu() - h_acc).abs().max()) <= 1e-12 * float(h_S.max())
    assert float((S[rows].cpu() - h_S).abs().max()) <= 1e-12 * float(h_S.max())
    return acc, S


def _check(name, pr, epi, got, ref, bound, which, tol=None):
    tol = R.maxnorm_tol(pr.fmt, pr.dtype, epi, which) if tol is None else tol
    rel = R.relerr(got, ref)
    nbad, ratio = R.violations(got, ref, bound)
    print(f"{name} {pr.fmt} {IDS[pr.dtype]} M={pr.M} N={pr.N} K={pr.K} epi {epi} {which}: max-norm {rel:.3e} (bound {tol:.1e}), "
          f"worst per-element error / bound {ratio:.3f}")
    assert rel < tol, (epi, which, rel, tol)
    assert nbad == 0, (epi, which, nbad, ratio)


def _run_case(name, fmt, dtype, M, N, K, dev, m_alloc=None, host_rows=128, epis=None):
    E = _E()
    pr = R.Problem(fmt, dtype, M, N, K, m_alloc=m_alloc)
    out_lo8 = 1 if fmt == "mixed" else 0
    epis = R.LEGAL_EPIS[fmt] if epis is None else epis
    for epi in epis:
        assert E.op_gemm_route(dtype, epi, R.A_SPLIT[fmt], M, N, K) == (_family(name),) + GEOMETRY[name], (name, epi)
    t = _device_operands(pr, dev)
    acc, S = _products(pr, dev, host_rows)
    for epi in epis:
        grad = epi in (R.EPI_GELUBWD, R.EPI_GELUBWD_SPLIT)
        ref = R.reference(epi, acc, S, pr.k_eff, dtype, bias=None if grad else t["bias"], resid=t["resid"], aux=t["aux"], out_lo8=out_lo8)
        for want_out2 in ((True, False) if epi in (R.EPI_GELU, R.EPI_GELU_SPLIT) else (False,)):
            out, o2 = _launch(pr, t, epi, want_out2, out_lo8, dev)
            _check(name, pr, epi, R.decode(out, epi, N, out_lo8), *ref["out"], "out")
            if want_out2:
                _check(name, pr, epi, o2.double(), *ref["out2"], "out2")
            again, o2b = _launch(pr, t, epi, want_out2, out_lo8, dev)
            assert torch.equal(out.view(torch.uint8), again.view(torch.uint8)), (epi, "second run differs")
            assert o2 is None or torch.equal(o2.view(torch.int16), o2b.view(torch.int16)), (epi, "second run differs (out2)")
        if epi == R.EPI_RESID32:      # in place: out aliases resid (the towers' residual stream)
            buf = t["resid"].clone()
            _launch(pr, t, epi, False, out_lo8, dev, out=buf, resid=buf)
            assert torch.equal(buf, out), "in-place residual differs from the out-of-place call"
        if epi == R.EPI_STORE32:      # padded A rows on THIS kernel's loader: the padding is never read, the result does not move
            padded, _ = _launch(pr, t, epi, False, out_lo8, dev, A=_padded_a(pr, dev), lda=pr.A.shape[1] + 64)
            assert bool(torch.isfinite(padded).all()), "the padding of A was read"
            assert torch.equal(padded, out), "lda changes the result"
        if epi == R.EPI_STORE_SPLIT:      # padded pair rows on this kernel's tile shape
            buf = torch.full((M, 2 * N + 64), SENTINEL, dtype=torch.int16, device=dev).view(dtype)
            buf[:, :2 * N] = 0
            _launch(pr, t, epi, False, out_lo8, dev, out=buf, ldo=2 * N + 64)
            assert bool((buf.view(torch.int16)[:, 2 * N:] == SENTINEL).all()), "the padding of the output was written"
            assert torch.equal(buf[:, :2 * N].view(torch.int16), out.view(torch.int16)), "ldo changes the result"
        if epi in (R.EPI_GELU_SPLIT, R.EPI_GELUBWD_SPLIT) and fmt != "single":
            # the other output format: a mixed A operand writing a hi|lo pair, a pair A operand writing a mixed pair.  Max-norm bound:
            # the mixed pair's own (2 x its resolution), resp. the mixed product's bound of the pair-writing epilogue 7
            other = 1 - out_lo8
            ref_o = R.reference(epi, acc, S, pr.k_eff, dtype, bias=None if grad else t["bias"], aux=t["aux"], out_lo8=other)
            out_o, _ = _launch(pr, t, epi, False, other, dev)
            _check(name, pr, epi, R.decode(out_o, epi, N, other), *ref_o["out"], f"out (out_lo8={other})",
                   tol=2 * R.MIXED_PAIR_TOL[dtype] if other else R.MIXED_GEMM_TOL[dtype])
    torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------------------------------------ the matrix on 32 compute units
MATRIX = [(r, f, K, mi) for r in R.ROUTES32 for f in R.FORMATS if not (r == "pc" and f == "single") for K in R.K_VALUES[f] for mi in range(3)]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("route,fmt,K,mi", MATRIX, ids=[f"{r}-{f}-K{K}-{('ragged', 'exact', 'plus1')[mi]}" for r, f, K, mi in MATRIX])
def test_gemm_matrix_32cu(route, fmt, K, mi, dtype, dev, stream32):
    spec = R.ROUTES32[route]
    with torch.cuda.stream(stream32):
        assert _E().device_cus(dev) >= 32 and int(_L().lib.mvlpt_stream_cus(stream32.cuda_stream)) == 32
        _run_case(route, fmt, dtype, spec[mi], spec[3], K, dev, m_alloc=max(spec[:3]))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("fmt", list(R.PHASED32))
@pytest.mark.parametrize("mi", range(3), ids=["ragged", "exact", "plus1"])
def test_gemm_phased_32cu(fmt, mi, dtype, dev, stream32):
    _, N, K = R.PHASED32[fmt]
    Ms = R.ROUTES32["pcp"][:3]
    with torch.cuda.stream(stream32):
        _run_case("phased", fmt, dtype, Ms[mi], N, K, dev, m_alloc=max(Ms))


# ------------------------------------------------------------------------------------------------ folded consumers: the two other rings
@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("cus,route,fmt,M,N,K,ntp", [(32, "r3", "single", 1400, 1152, 256, 2), (32, "r3", "pair", 1400, 1152, 256, 2),
                                                     (32, "r3", "mixed", 1281, 1152, 256, 2), (32, "r3", "single", 1536, 1152, 256, 2),
                                                     (32, "r4", "pair", 391, 512, 1024, 8), (32, "r4", "mixed", 391, 512, 1024, 8),
                                                     (32, "r4", "pair", 385, 512, 256, 8), (32, "r4", "mixed", 512, 512, 128 * 3, 8),
                                                     # the whole device: 387 tiles of 256x128 (1.5 rounds); 72 tiles of 128x128
                                                     (256, "r3", "single", 10951, 1152, 256, 2), (256, "r4", "pair", 1100, 1024, 256, 8)])
def test_gemm_folded_rings(cus, route, fmt, M, N, K, ntp, dtype, dev, stream32):
    """gemm_bt_kernel's 3-deep 256x128 ring (folded consumer with 2-slot rows) and its 4-deep 128x128 ring (pair operands, at most one tile
    per compute unit, folded: gemm_pc_kernel does not fold), through mvlpt_op_gemm_folded with seeded partial sums."""
    E = _E()
    pr = R.Problem(fmt, dtype, M, N, K)
    nt = K // 128
    g = torch.Generator().manual_seed(M + K)
    # partial sums of rows with mean ~0.3 and variance ~1 (any consistent {s1, s2} is a legal input of the consumer)
    mean = 0.3 * torch.randn(M, generator=g)
    var = 0.5 + torch.rand(M, generator=g)
    s1, s2 = mean * K, (var + mean * mean) * K
    w = torch.rand(M, nt, generator=g) + 0.5
    w = w / w.sum(1, keepdim=True)
    part = torch.zeros(M, ntp, 2)
    part[:, :nt, 0], part[:, :nt, 1] = w * s1.view(-1, 1), w * s2.view(-1, 1)
    colsum = torch.randn(N, generator=g)
    out_lo8 = 1 if fmt == "mixed" else 0
    epis = [R.EPI_STORE16, R.EPI_GELU, R.EPI_GELU_SPLIT, R.EPI_STORE_SPLIT] if fmt != "mixed" else [R.EPI_GELU_SPLIT, R.EPI_STORE_SPLIT]
    assert cus == 32 or E.device_cus(dev) == 256, "the whole-device shapes are chosen for 256 compute units"
    with torch.cuda.stream(stream32 if cus == 32 else torch.cuda.default_stream(dev)):
        for epi in epis:
            assert E.op_gemm_route(dtype, epi, R.A_SPLIT[fmt], M, N, K, fold_ntp=ntp) == (_family(route),) + GEOMETRY[route], epi
        t = _device_operands(pr, dev)
        part_d, cs_d = part.to(dev), colsum.to(dev)
        acc, S = _products(pr, dev)
        v, e_v = R.folded_linear(acc, S, pr.k_eff, K, part_d, nt, cs_d, t["bias"])
        for epi in epis:
            ref = R.finish(epi, v, e_v, dtype, out_lo8=out_lo8)
            gelu = epi in (R.EPI_GELU, R.EPI_GELU_SPLIT)
            run = lambda: E.op_gemm_folded(t["A"], t["Bt"], cs_d, t["bias"], part_d, nt, epi=epi, a_split=R.A_SPLIT[fmt], ldb=pr.ldb,
                                           w8_exp=pr.w8_exp, out2=gelu)
            res = run()
            out, o2 = res if gelu else (res, None)
            lo8 = out_lo8 if epi == R.EPI_GELU_SPLIT else 0
            nbad, ratio = R.violations(R.decode(out, epi, N, lo8), *ref["out"])
            rel = R.relerr(R.decode(out, epi, N, lo8), ref["out"][0])
            print(f"{route} folded {fmt} {IDS[dtype]} M={M} K={K} epi {epi}: max-norm {rel:.3e}, worst per-element error / bound {ratio:.3f}")
            assert nbad == 0, (epi, nbad, ratio)
            # max-norm: the project's bound of this epilogue and format, and tests/test_hip_fold.py's for folded fp16 pair / mixed operands
            tol = R.maxnorm_tol(fmt, dtype, epi)
            if dtype == torch.float16 and fmt != "single" and epi in (R.EPI_GELU_SPLIT, R.EPI_STORE_SPLIT):
                tol = min(tol, 2e-5 if fmt == "pair" else 1e-4)
            assert rel < tol, (epi, rel, tol)
            if gelu:
                assert R.violations(o2.double(), *ref["out2"])[0] == 0 and R.relerr(o2, ref["out2"][0]) < R.TOL[dtype]
            res2 = run()
            out_b = res2[0] if gelu else res2
            assert torch.equal(out.view(torch.int16), out_b.view(torch.int16))
        torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------------------------------------ one case per family on the whole device
@pytest.mark.parametrize("route,fmt,M,N,K", [("pcp", "pair", 10951, 1152, 256), ("big_one", "single", 3900, 3072, 128),
                                             ("big_multi", "mixed", 21900, 3072, 128), ("phased", "single", 10951, 1152, 2048),
                                             ("small", "pair", 4300, 1024, 64), ("pc", "mixed", 1100, 1024, 128)])
def test_gemm_whole_device(route, fmt, M, N, K, dev):
    """The smallest ragged shape that reaches each kernel on all compute units; the host's float64 matmul checks the last 2048 rows of
    the device's."""
    if _E().device_cus(dev) != 256:
        pytest.fail("the whole-device shapes are chosen for 256 compute units")
    _run_case(route, fmt, torch.float16, M, N, K, dev, host_rows=2048)


# ------------------------------------------------------------------------------------------------ row pitches
@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS.values())
@pytest.mark.parametrize("fmt", ["pair", "mixed"])
@pytest.mark.parametrize("d,M", [(512, 300), (768, 391)])
def test_gemm_row_pitches(d, M, fmt, dtype, dev):
    """The padded rows every real CLIP width gets (wide_pitch(): MLP pair tensors of 16 d bytes): lda = 2K + 64 on the down-projection's
    A operand, ldo = 2N + 64 on the pair the up-projection (5), its backward (6) and a plain pair store (7) write.  A's padding (and the
    unused quarter of a mixed row) holds NaNs, the output's padding a sentinel; results are bit-identical to the dense call."""
    E = _E()
    out_lo8 = 1 if fmt == "mixed" else 0
    # ---- lda: [M, 4d] pair -> [M, d]
    pr = R.Problem(fmt, dtype, M, d, 4 * d)
    K = pr.K
    t = _device_operands(pr, dev)
    wide = R.with_pitch(pr.A, 2 * K + 64, NAN16[dtype])
    if fmt == "mixed":
        wide.view(torch.int16)[:, K + K // 2:2 * K] = NAN16[dtype]
    wide = wide.to(dev)
    for epi in (R.EPI_RESID32, R.EPI_STORE32, R.EPI_STORE_SPLIT):
        assert E.op_gemm_route(dtype, epi, R.A_SPLIT[fmt], M, d, K)[0] > 0
        dense, _ = _launch(pr, t, epi, False, out_lo8, dev)
        padded, _ = _launch(pr, t, epi, False, out_lo8, dev, A=wide, lda=2 * K + 64)
        assert bool(torch.isfinite(padded.float()).all()), "the padding of A was read"
        assert torch.equal(dense.view(torch.uint8), padded.view(torch.uint8)), (epi, "lda changes the result")
    # ---- ldo: [M, d] -> pair [M, 2 * 4d]
    pr = R.Problem(fmt, dtype, M, 4 * d, d)
    N = pr.N
    t = _device_operands(pr, dev)
    acc, S = _products(pr, dev)
    for epi in (R.EPI_GELU_SPLIT, R.EPI_GELUBWD_SPLIT, R.EPI_STORE_SPLIT):
        dense, u_dense = _launch(pr, t, epi, epi == R.EPI_GELU_SPLIT, out_lo8, dev)
        buf = torch.full((M, 2 * N + 64), SENTINEL, dtype=torch.int16, device=dev).view(dtype)
        buf[:, :2 * N] = 0
        padded, u_padded = _launch(pr, t, epi, epi == R.EPI_GELU_SPLIT, out_lo8, dev, out=buf, ldo=2 * N + 64)
        assert bool((padded.view(torch.int16)[:, 2 * N:] == SENTINEL).all()), (epi, "the padding of the output was written")
        assert torch.equal(padded[:, :2 * N].view(torch.int16), dense.view(torch.int16)), (epi, "ldo changes the result")
        assert u_dense is None or torch.equal(u_dense.view(torch.int16), u_padded.view(torch.int16))
        grad = epi == R.EPI_GELUBWD_SPLIT
        ref = R.reference(epi, acc, S, pr.k_eff, dtype, bias=None if grad else t["bias"], aux=t["aux"], out_lo8=out_lo8)
        _check("pitch", pr, epi, R.decode(padded, epi, N, out_lo8), *ref["out"], "out")
    torch.cuda.current_stream().synchronize()


def test_gemm_pitch_refusals(dev):
    E = _E()
    pr = R.Problem("pair", torch.float16, 130, 256, 128)
    t = _device_operands(pr, dev)
    wide = R.with_pitch(pr.A, 2 * 128 + 64, 0).to(dev)
    out = torch.zeros(130, 2 * 256 + 64, device=dev, dtype=torch.float16)
    _launch(pr, t, R.EPI_STORE_SPLIT, False, 0, dev, A=wide, lda=320, out=out, ldo=576)       # the legal call
    for epi, kw in [(R.EPI_STORE_SPLIT, dict(lda=2 * 128 - 8)),        # lda shorter than the pair's row
                    (R.EPI_STORE_SPLIT, dict(lda=2 * 128 + 4)),        # not a multiple of 8
                    (R.EPI_STORE_SPLIT, dict(ldo=2 * 256 + 4)),
                    (R.EPI_STORE_SPLIT, dict(ldo=2 * 256 - 8)),
                    (R.EPI_STORE32, dict(ldo=2 * 256 + 64)),           # ldo on an epilogue that writes no pair
                    (R.EPI_STORE16, dict(ldo=2 * 256 + 64))]:
        with pytest.raises(RuntimeError):
            _launch(pr, t, epi, False, 0, dev, A=wide, out=out, **kw)
    sp = R.Problem("single", torch.float16, 130, 256, 128)
    with pytest.raises(RuntimeError):
        _launch(sp, _device_operands(sp, dev), R.EPI_STORE16, False, 0, dev, lda=120)         # lda < K
    with pytest.raises(RuntimeError):
        E.op_gemm_route(torch.float16, R.EPI_STORE16, 2, 130, 256, 128)                        # no mixed pair with a 16-bit epilogue
    torch.cuda.current_stream().synchronize()
