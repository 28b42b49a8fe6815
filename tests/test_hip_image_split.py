"""The per-stream grid cap (mvlpt_stream_set_cu_cap) and the image forward in two enqueues (mvlpt_image_fwd_begin / _resume), and the
trainer's prefetch split on top of them.  Everything here is an equality bit for bit: the cap only changes how many workgroups a
persistent / grid-stride launch has, the split only where the tower's launch sequence is cut."""
import contextlib
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@contextlib.contextmanager
def side_stream(cap=0):
    """A side stream with the grid cap set while the body enqueues on it; synchronised and uncapped on exit."""
    from mvlpt_amd import engine as E
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    E.set_stream_cu_cap(st, cap)
    try:
        with torch.cuda.stream(st):
            yield st
    finally:
        E.set_stream_cu_cap(st, 0)
        st.synchronize()


def under_caps(fn, caps):
    """fn() on an uncapped side stream and under every cap -> [(cap, result)], results moved to the host."""
    out = []
    for cap in (0,) + tuple(caps):
        with side_stream(cap):
            r = fn()
        torch.cuda.synchronize()
        out.append((cap, [t.cpu() for t in (r if isinstance(r, (tuple, list)) else (r,)) if isinstance(t, torch.Tensor)]))
    return out


def assert_all_equal(runs, what):
    base = runs[0][1]
    for cap, res in runs[1:]:
        assert len(res) == len(base)
        for i, (a, b) in enumerate(zip(base, res)):
            assert not torch.isnan(a.float()).any(), f"{what}: NaN in output {i}"
            assert torch.equal(a, b), f"{what}: output {i} under cap {cap} differs from the uncapped launch"


# ------------------------------------------------------------------------------------------------ the cap itself
def test_stream_cus_reports_the_cap_and_the_device_again():
    from mvlpt_amd import _lib
    from mvlpt_amd import engine as E
    dev_cus = E.device_cus(torch.device("cuda:0"))
    st = torch.cuda.Stream()
    assert E.stream_cus(st) == dev_cus
    E.set_stream_cu_cap(st, 16)
    assert E.stream_cus(st) == 16
    assert E.stream_cus(torch.cuda.Stream()) == dev_cus          # another stream is not capped
    E.set_stream_cu_cap(st, 13)                                  # not a multiple of 8: the next lower multiple
    assert E.stream_cus(st) == 8
    E.set_stream_cu_cap(st, 10 ** 6)                             # above the device: the device
    assert E.stream_cus(st) == dev_cus
    E.set_stream_cu_cap(st, 0)
    assert E.stream_cus(st) == dev_cus
    E.set_stream_cu_cap(st, 24)
    E.set_stream_cu_cap(st, -1)
    assert E.stream_cus(st) == dev_cus
    assert _lib.lib.mvlpt_stream_set_cu_cap(C.c_void_p(st.cuda_stream), 5) == _lib.ERR_ARG      # below one CU per XCD
    assert _lib.lib.mvlpt_stream_set_cu_cap(None, 8) == _lib.ERR_ARG
    assert E.stream_cus(st) == dev_cus


def _gemm_inputs(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * 0.5).half().to(DEV)
    W = (torch.randn(N, K, generator=g) * 0.05).half().to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    return A, W, b


def _route(cap, epi, a_split, M, N, K):
    """(family, tile_m, tile_n) of the kernel a GEMM enqueued under `cap` runs (0: uncapped): the router sees the capped count."""
    from mvlpt_amd import engine as E
    with side_stream(cap):
        fam, tm, tn, _ = E.op_gemm_route(torch.float16, epi, a_split, M, N, K)
    return fam, tm, tn


def test_capped_gemm_256x256_issue_shape():
    """M = N = 768, K = 128.  The router counts tile rounds per compute unit of the stream, so the cap also moves the geometry: 18 tiles
    of 256x128 are more than 1.5 rounds of 8 workgroups (the persistent kernel with movers: two full rounds and a ragged third of
    two tiles), but under cap 16 and uncapped the problem stays on 128x128 tiles.  All three agree bit for bit."""
    from mvlpt_amd import _lib
    from mvlpt_amd import engine as E
    A, W, b = _gemm_inputs(768, 768, 128, 1)
    for epi in (_lib.EPI_STORE16, _lib.EPI_STORE32):
        assert _route(8, epi, 0, 768, 768, 128) == (_lib.GEMM_PCP, 256, 128)
        assert _route(16, epi, 0, 768, 768, 128) == _route(0, epi, 0, 768, 768, 128) == (_lib.GEMM_BT_128x128_R2, 128, 128)
        runs = under_caps(lambda: E.op_gemm(A, W, epi, bias=b), (8, 16))
        assert_all_equal(runs, f"gemm 768x768x128 epi {epi}")


def test_capped_gemm_reaches_the_256x256_kernel():
    """The 256x256 geometry under a cap, both ways its persistent walk can end.  M = 1280, N = 1024, K = 2048 under cap 8: 20 tiles,
    two full rounds in XCD order and a ragged third of four tiles in plain order (cap 16 sends the shape to the phased 256x128
    kernel, no cap to 128x128 tiles).  M = 768, N = 1024, K = 128 under cap 16: 12 tiles fill one round to 75 %, fewer tiles than
    workgroups, a grid of 12."""
    from mvlpt_amd import _lib
    from mvlpt_amd import engine as E
    epi = _lib.EPI_STORE32
    M, N, K = 1280, 1024, 2048
    A, W, b = _gemm_inputs(M, N, K, 2)
    assert _route(8, epi, 0, M, N, K) == (_lib.GEMM_BT_256x256_R2, 256, 256)
    assert _route(16, epi, 0, M, N, K) == (_lib.GEMM_PHASED, 256, 128)
    assert _route(0, epi, 0, M, N, K) == (_lib.GEMM_BT_128x128_R2, 128, 128)
    assert_all_equal(under_caps(lambda: E.op_gemm(A, W, epi, bias=b), (8, 16)), "gemm 1280x1024x2048")
    M, N, K = 768, 1024, 128
    A, W, b = _gemm_inputs(M, N, K, 8)
    assert _route(16, epi, 0, M, N, K) == (_lib.GEMM_BT_256x256_R2, 256, 256)
    assert_all_equal(under_caps(lambda: E.op_gemm(A, W, epi, bias=b), (8, 16)), "gemm 768x1024x128")


def test_capped_gemm_pcp_shape():
    """N = K = 768, M = 1024 under cap 8: 24 tiles of 256x128 = 3 rounds, the persistent kernel with data-movement waves."""
    from mvlpt_amd import _lib
    from mvlpt_amd import engine as E
    M, N, K = 1024, 768, 768
    A, W, b = _gemm_inputs(M, N, K, 3)
    resid = torch.randn(M, N, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert _route(8, _lib.EPI_RESID32, 0, M, N, K) == (_lib.GEMM_PCP, 256, 128)
    runs = under_caps(lambda: E.op_gemm(A, W, _lib.EPI_RESID32, bias=b, resid=resid), (8,))
    assert_all_equal(runs, "gemm_pcp 1024x768x768")
    runs = under_caps(lambda: E.op_gemm(A, W, _lib.EPI_GELU, bias=b), (8, 12))           # 12 behaves as 8
    assert_all_equal(runs, "gemm_pcp 1024x768x768 gelu")


def test_capped_gemm_pc_one_tile_shape():
    """M = 300, N = 512, K = 512 on a mixed pair: 12 tiles of 128x128.  gemm_pc takes a problem with no more tiles than compute
    units, one tile per workgroup: uncapped and under cap 16.  Under cap 8 the 12 tiles no longer fit and the launch is the
    persistent 128x128 kernel (two workgroups per compute unit)."""
    from mvlpt_amd import _lib
    from mvlpt_amd import engine as E
    M, N, K = 300, 512, 512
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(M, K, generator=g) * 0.5).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    A2 = E.op_cast_mixed(x, torch.float16)
    Wp, e8 = E.op_pack_weight_mixed(w, torch.float16)
    torch.cuda.synchronize()
    epi = _lib.EPI_STORE32
    assert _route(0, epi, 2, M, N, K)[0] == _route(16, epi, 2, M, N, K)[0] == _lib.GEMM_PC
    assert _route(8, epi, 2, M, N, K) == (_lib.GEMM_BT_128x128_R2, 128, 128)
    runs = under_caps(lambda: E.op_gemm_mixed(A2, Wp, e8, epi, bias=b), (8, 16))
    assert_all_equal(runs, "gemm_pc 300x512x512 mixed")


@pytest.mark.parametrize("N", [2, 43])
def test_capped_persistent_attention_forward(N):
    """L = 197, 12 heads.  The launcher picks the persistent kernel by the stream's compute units WITHOUT the cap (the persistent
    kernel and the one-workgroup-per-head kernel differ in the last bit) and sizes its grid WITH it.  2 images = 24 items: one
    workgroup per item under every cap.  43 images = 516 items, two per compute unit of the device: the persistent kernel on grids
    of 8 (64.5 items per workgroup: a ragged walk), 16 and the whole chip."""
    from mvlpt_amd import engine as E
    L, H = 197, 12
    qkv = (torch.randn(N * L, 3 * H * 64, generator=torch.Generator().manual_seed(6)) * 0.7).half().to(DEV)
    runs = under_caps(lambda: E.op_attention_fwd(qkv, N, L, H, False), (8, 16))
    assert_all_equal(runs, f"attention forward, {N * H} items")


def test_capped_layernorm_forward_and_backward():
    """300 rows: 75 workgroups of 4 rows uncapped, a grid-stride walk of 64 under cap 8."""
    from mvlpt_amd import engine as E
    rows, d = 300, 768
    g = torch.Generator().manual_seed(7)
    x = torch.randn(rows, d, generator=g).to(DEV)
    gamma, beta = torch.randn(d, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV)
    dy = torch.randn(rows, d, generator=g).half().to(DEV)
    resid = torch.randn(rows, d, generator=g).to(DEV)
    assert_all_equal(under_caps(lambda: E.op_layernorm_fwd(x, gamma, beta, torch.float16), (8,)), "layernorm forward")
    assert_all_equal(under_caps(lambda: E.op_layernorm_bwd(dy, x, gamma, resid=resid), (8,)), "layernorm backward")


# ------------------------------------------------------------------------------------------------ split == whole
@pytest.fixture(scope="module")
def vitb32():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS, make_state_dict
    arch = ARCHS["ViT-B/32"]
    eng = Engine.from_state_dict(make_state_dict(arch, 2), "fp16")
    eng.set_ln_fold(1, 1)                     # B = 4 is 200 token rows: force the folded tower on
    g = torch.Generator().manual_seed(11)
    image = torch.randn(4, 3, arch.image_resolution, arch.image_resolution, generator=g).half().to(DEV)
    yield eng, arch, image
    eng.close()


def _split_fwd(eng, image, stop, cap=8, **kw):
    """First part under `cap` on a side stream, second part uncapped on the main stream."""
    with side_stream(cap) as st:
        eng.image_fwd_begin(image, stop_block=stop, **kw)
    torch.cuda.current_stream().wait_stream(st)
    return eng.image_fwd_resume()


@pytest.mark.parametrize("packed", [True, False])
def test_split_forward_equals_whole(vitb32, packed):
    eng, arch, image = vitb32
    eng.set_resid_packed(packed)
    try:
        whole = eng.image_fwd(image)
        torch.cuda.synchronize()
        assert torch.isfinite(whole).all()
        for stop in (0, 1, arch.vision_layers - 1, arch.vision_layers):
            got = _split_fwd(eng, image, stop)
            torch.cuda.synchronize()
            assert torch.equal(got, whole), f"packed={packed} stop_block={stop}"
        assert torch.equal(eng.image_fwd(image), whole)
    finally:
        eng.set_resid_packed(True)


@pytest.mark.parametrize("n_deep,precision", [(11, "split_grad"), (4, "split_grad"), (11, "split_all")], ids=["11", "4", "11-split_all"])
def test_split_forward_with_deep_prompts_and_backward(vitb32, n_deep, precision):
    """n_deep = 11: every later block has its prompt rows overwritten, the last one is CLS-only.  n_deep = 4: blocks 5 .. 11 are
    skipped (the reference's quirk), activations copied through for the backward; the cut falls in front of, at the edge of and
    inside the skipped range.  split_all: 16-bit pair operands instead of the default's mixed pairs, through the full-width blocks
    and the CLS-only last block, forward and backward."""
    eng, arch, image = vitb32
    assert arch.vision_layers == 12
    eng.set_precision(precision)
    try:
        _split_deep_prompts_and_backward(eng, arch, image, n_deep)
    finally:
        eng.set_precision("split_grad")


def _split_deep_prompts_and_backward(eng, arch, image, n_deep):
    g = torch.Generator().manual_seed(12)
    dv = arch.vision_width
    vpt = (torch.randn(3, dv, generator=g) * 0.1).to(DEV)
    deep = (torch.randn(n_deep, 3, dv, generator=g) * 0.1).to(DEV)
    dfeat = torch.randn(4, arch.embed_dim, generator=g).to(DEV)
    whole = eng.image_fwd(image, vpt, deep, save_for_bwd=True)
    dvpt0, ddeep0 = eng.image_bwd(dfeat)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and torch.isfinite(dvpt0).all() and torch.isfinite(ddeep0).all()
    for stop in (0, 1, 3, 5, 7, arch.vision_layers - 1, arch.vision_layers):
        got = _split_fwd(eng, image, stop, vpt=vpt, vpt_deep=deep, save_for_bwd=True)
        dvpt, ddeep = eng.image_bwd(dfeat)
        torch.cuda.synchronize()
        assert torch.equal(got, whole), stop
        assert torch.equal(dvpt, dvpt0) and torch.equal(ddeep, ddeep0), stop


def test_state_errors_touch_nothing(vitb32):
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import _ptr, _stream
    eng, arch, image = vitb32
    lib, h = _lib.lib, eng.h
    whole = eng.image_fwd(image)
    feat = torch.full_like(whole, float("nan"))
    dfeat = torch.ones_like(whole)
    torch.cuda.synchronize()
    begin = lambda: lib.mvlpt_image_fwd_begin(h, _ptr(image), _lib.DT_F16, None, None, 0, 0, image.shape[0], 0, 2, _stream())
    assert lib.mvlpt_image_fwd_resume(h, _ptr(feat), _stream()) == _lib.ERR_STATE          # resume without begin
    assert "image_fwd_begin" in _lib.last_error(h)
    assert begin() == 0
    assert begin() == _lib.ERR_STATE                                                       # a second begin before resume
    assert lib.mvlpt_image_bwd(h, _ptr(dfeat), None, None, _stream()) == _lib.ERR_STATE     # a backward in between
    assert lib.mvlpt_image_fwd(h, _ptr(image), _lib.DT_F16, None, None, 0, 0, image.shape[0], _ptr(feat), 0, _stream()) == _lib.ERR_STATE
    torch.cuda.synchronize()
    assert torch.isnan(feat).all()                                                         # none of them wrote the output
    assert lib.mvlpt_image_fwd_resume(h, _ptr(feat), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(feat, whole)
    assert lib.mvlpt_image_fwd_resume(h, _ptr(feat), _stream()) == _lib.ERR_STATE
    # an abandoned begin leaves a usable engine
    assert begin() == 0 and lib.mvlpt_image_fwd_abandon(h) == 0
    assert lib.mvlpt_image_fwd_resume(h, _ptr(feat), _stream()) == _lib.ERR_STATE
    assert torch.equal(_split_fwd(eng, image, 1), whole)
    assert torch.equal(eng.image_fwd(image), whole)


# ------------------------------------------------------------------------------------------------ trainer
def _run_three_steps(tmp_path, split, overlap=True, pipelining=True):
    from tests.test_hip_trainer import make_trainer
    torch.manual_seed(0)
    tr = make_trainer(tmp_path, "coop", steps=3, pipelining=pipelining)
    tr.cfg.TRAIN.PRINT_FREQ = 10 ** 9
    tr.model.prefetch_split = split
    tr.model.overlap_towers = overlap
    eng = tr.model.engine
    calls = {"begin": 0, "resume": 0, "whole": 0}
    for name, attr in (("begin", "image_fwd_begin"), ("resume", "image_fwd_resume"), ("whole", "image_fwd")):
        orig = getattr(eng, attr)
        setattr(eng, attr, lambda *a, _o=orig, _n=name, **k: (calls.__setitem__(_n, calls[_n] + 1), _o(*a, **k))[1])
    out = tr.run_epoch()
    torch.cuda.synchronize()
    params = {k: v.detach().cpu().clone() for k, v in tr.model.prompt_learner.named_parameters()}
    return tr, calls, (out["loss"].cpu(), torch.as_tensor(out["acc"]).cpu()), params


def test_trainer_prefetch_split_is_transparent_and_inert(tmp_path):
    _, calls0, out0, p0 = _run_three_steps(tmp_path, (0, 0))
    assert calls0 == {"begin": 0, "resume": 0, "whole": 3}
    tr, calls1, out1, p1 = _run_three_steps(tmp_path, (1, 8))
    # step 0 runs its own tower and prefetches batch 1 in one piece; step 1 begins batch 2 ahead of its forward and resumes it
    assert calls1 == {"begin": 1, "resume": 1, "whole": 2}, calls1
    assert not tr.model.prefetch.begun and not tr.model.prefetch.finished
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])
    assert set(p0) == set(p1)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    # inert where today's prefetch is inert
    for kw in ({"overlap": False}, {"pipelining": False}):
        _, calls, out, p = _run_three_steps(tmp_path, (1, 8), **kw)
        assert calls["begin"] == 0 and calls["resume"] == 0 and calls["whole"] == 3, (kw, calls)
        assert torch.equal(out0[0], out[0])
        for k in p0:
            assert torch.equal(p0[k], p[k]), (kw, k)


def test_split_point_past_the_tower_is_inert(tmp_path):
    """The shipped default applies to the backbones it was measured on, and a split point past the last full-width block of a tower
    is no split of that tower: the two-block test tower stays in one piece either way."""
    from tests.test_hip_trainer import make_trainer
    tr = make_trainer(tmp_path, "coop", steps=3)
    assert tr.model.prefetch_split == (0, 0) and not tr.model.split_active()
    tr.model.prefetch_split = (tr.model.engine.arch.vision_layers, 8)
    assert not tr.model.split_active()
    tr.model.prefetch_split = (tr.model.engine.arch.vision_layers - 1, 8)
    assert tr.model.split_active()
    tr.model.overlap_towers = False
    assert not tr.model.split_active()


def test_begin_without_resume_leaves_no_stale_workspace(tmp_path):
    from tests.test_hip_trainer import make_trainer
    torch.manual_seed(0)
    tr = make_trainer(tmp_path, "coop", steps=3)
    tr.model.prefetch_split = (1, 8)
    model, eng = tr.model, tr.model.engine
    img_a, img_b = (tr.parse_batch_train(tr.train_loader_x[i])[0] for i in (0, 1))
    want_a, want_b = eng.image_fwd(img_a).clone(), eng.image_fwd(img_b).clone()
    with torch.no_grad():
        logits_b = model(img_b).clone()
    torch.cuda.synchronize()
    # the loop leaves the loader after the first part of batch a's tower: the trainer's epilogue gives it up
    assert model.prefetch_image_features(img_a, stop_block=1, cu_cap=8) and model.prefetch.begun
    tr.end_of_epoch_loop()
    assert not model.prefetch.begun and not eng.image_fwd_pending()
    assert torch.equal(eng.image_fwd(img_b), want_b)
    # ... and a forward that meets a tower begun for another tensor finishes that one first, then runs its own
    assert model.prefetch_image_features(img_a, stop_block=1, cu_cap=8)
    with torch.no_grad():
        got = model(img_b)
    torch.cuda.synchronize()
    assert torch.equal(got, logits_b)
    assert not model.prefetch.begun and model.has_prefetched(img_a)
    feat_a, ev = model.prefetch.get(img_a).features, model.prefetch.get(img_a).ready
    ev.synchronize()
    assert torch.equal(feat_a, want_a)
    model.drop_prefetch()
