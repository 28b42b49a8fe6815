"""Nearest vocabulary tokens on the device (-m gpu): mvlpt_op_nearest_rows / mvlpt_nearest_tokens / Engine.nearest_tokens and the
interpretation methods of the trainers, against the float64 oracle of tests/nearest_ref.py.

Every index is compared exactly and every distance inside the derived bound (d / 2 + 3) * 2^-24 * D64; where indices are compared
the oracle's neighbours are first shown to be more than 8 tolerances apart (planted rows), so the comparison cannot hinge on rounding.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nearest_ref as N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL_I, SENTINEL_F = -77, -12345.0

# (V, d, R, k): the smallest at which each part can go wrong; seeds follow the list order
PLANTED = [
    (257, 4, 5, 3),           # smallest d, V no tile multiple, R below one row tile
    (1003, 64, 17, 8),        # odd V, R one past a tile
    (4097, 128, 48, 16),      # CSC-like, 3 classes x 16
    (49408, 512, 16, 5),      # the real table
    (49408, 768, 16, 64),     # ViT-L text width, maximum k
]
LARGE_R = (4097, 128, 300, 5)
UNPLANTED = [(1, 4, 1, 1), (3, 8, 2, 3), (70, 8, 1, 64)]     # k == V; every vocabulary slice holds fewer than k tokens


def run(Q, E, k):
    from mvlpt_amd.engine import op_nearest_rows
    idx, dist = op_nearest_rows(torch.tensor(Q).to(DEV), torch.tensor(E).to(DEV), k)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def check_planted(seed, V, d, R, k, call):
    Q, E, ids, D = N.inputs(seed, V, d, R, k)
    want = N.assert_separated(D, ids, k, d)                      # the oracle alone, before the GPU is looked at
    idx, dist = call(Q, E, k)
    assert idx.shape == (R, k) and dist.shape == (R, k)
    assert np.array_equal(idx, want)
    worst = N.assert_dist_inside(dist, np.take_along_axis(D, want, axis=1), d)
    print(f"V {V} d {d} R {R} k {k}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("seed,shape", list(enumerate(PLANTED)), ids=[str(s) for s in PLANTED])
def test_planted_neighbours_exact_indices_and_bounded_distances(seed, shape):
    check_planted(seed, *shape, run)


def test_large_r_at_kernel_level():
    check_planted(len(PLANTED), *LARGE_R, run)


@pytest.mark.parametrize("shape", UNPLANTED, ids=[str(s) for s in UNPLANTED])
def test_unplanted_by_distance(shape):
    V, d, R, k = shape
    Q, E, _, D = N.inputs(100 + V, V, d, R, k, planted=False)
    idx, dist = run(Q, E, k)
    want = np.sort(D, axis=1)[:, :k]                              # the j-th smallest float64 distance
    N.assert_dist_inside(dist, want, d)
    N.assert_dist_inside(np.take_along_axis(D, idx.astype(np.int64), axis=1), want, d, "D64 at the returned index")
    assert idx.min() >= 0 and idx.max() < V
    assert all(len(set(row.tolist())) == k for row in idx)


def test_ties_go_to_the_smaller_index_with_equal_bits():
    V, d, R, k = 1003, 64, 17, 8
    Q, E0, ids, _ = N.inputs(1, V, d, R, k)
    E = E0.copy()
    src, taken = [], set(ids.reshape(-1).tolist())
    for r in (0, 5, 16):                                          # several t among a row's nearest: t + 37 becomes a bitwise copy
        for j in range(4):
            t = int(ids[r, j])
            if t + 37 < V and t + 37 not in taken:
                E[t + 37] = E[t]
                taken.add(t + 37)
                src.append((t, r))
    assert len(src) >= 6
    idx, dist = run(Q, E, k)
    want = N.topk64(N.dist64(Q, E), k)                            # stable: the smaller index first
    assert np.array_equal(idx, want)
    for t, r in src:
        row = idx[r].tolist()
        a = row.index(t)
        assert row[a + 1] == t + 37
        assert dist[r, a].tobytes() == dist[r, a + 1].tobytes()


def test_a_copy_of_a_table_row_is_at_exactly_zero():
    V, d, R, k = 1003, 64, 17, 8
    Q0, E, _, _ = N.inputs(1, V, d, R, k)
    Q = Q0.copy()
    Q[3], Q[16] = E[0], E[V - 1]
    idx, dist = run(Q, E, k)
    assert idx[3, 0] == 0 and idx[16, 0] == V - 1
    assert dist[3, 0] == 0.0 and dist[16, 0] == 0.0 and not np.signbit(dist[[3, 16], 0]).any()
    assert (dist[:, 1:] > 0).all()


def test_nan_and_inf_rows_and_nan_table_rows():
    V, d, R, k = 1003, 64, 17, 8
    Q0, E0, ids, _ = N.inputs(1, V, d, R, k)
    base_idx, base_dist = run(Q0, E0, k)
    Q = Q0.copy()
    Q[2, 5], Q[9, :] = np.nan, np.inf
    idx, dist = run(Q, E0, k)
    for r in (2, 9):
        assert idx[r].tolist() == list(range(k))
    assert np.isnan(dist[2]).all() and np.isposinf(dist[9]).all()
    rest = [r for r in range(R) if r not in (2, 9)]
    assert np.array_equal(idx[rest], base_idx[rest]) and dist[rest].tobytes() == base_dist[rest].tobytes()
    # a table row holding a NaN is behind every number: never among a finite query's results while V - 1 >= k
    E = E0.copy()
    poisoned = [int(ids[0, 0]), int(ids[4, 1]), 0, V - 1]
    E[poisoned, 7] = np.nan
    idx, dist = run(Q0, E, k)
    assert not np.isin(idx, poisoned).any() and np.isfinite(dist).all()
    D = N.dist64(Q0, E)
    D[np.isnan(D)] = np.inf
    assert np.array_equal(idx, N.topk64(D, k))
    # ... and comes last, NaNs by index, when the table has nothing else left: V = k
    Es = E0[:k].copy()
    Es[[1, 4], 0] = np.nan
    idx, dist = run(Q0[:3], Es, k)
    assert (idx[:, -2:] == [1, 4]).all() and np.isnan(dist[:, -2:]).all() and np.isfinite(dist[:, :-2]).all()


def test_results_do_not_depend_on_the_grid():
    from mvlpt_amd.engine import op_nearest_rows, set_stream_cu_cap, stream_cus
    V, d, R, k = 20000, 64, 5, 8                                 # 40 token tiles: 40 slices uncapped, 20 under a cap of 8 units
    Q, E, _, _ = N.inputs(7, V, d, R, k)
    q, e = torch.tensor(Q).to(DEV), torch.tensor(E).to(DEV)
    st = torch.cuda.Stream(device=DEV)
    outs = []
    with torch.cuda.stream(st):
        full = stream_cus(st)
        for cap in (0, 8, 0):
            set_stream_cu_cap(st, cap)
            assert stream_cus(st) == (8 if cap else full)
            idx, dist = op_nearest_rows(q, e, k)
            st.synchronize()
            outs.append((idx.cpu().numpy(), dist.cpu().numpy()))
        set_stream_cu_cap(st, 0)
    for idx, dist in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and dist.tobytes() == outs[0][1].tobytes()


# ------------------------------------------------------------------------------------------------ refusals (host checks only)
def _raw_call(q, e, R, V, d, k, idx, dist, ws, ws_bytes):
    from mvlpt_amd._lib import lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    return lib.mvlpt_op_nearest_rows(p(q), p(e), R, V, d, k, p(idx), p(dist), p(ws), ws_bytes, None)


def test_refusals_launch_nothing_and_leave_the_outputs():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import nearest_workspace_bytes
    V, d, R, k = 257, 8, 5, 3
    q, e = torch.zeros(R, 1032, device=DEV), torch.zeros(V, 1032, device=DEV)      # wide enough for every d below
    idx = torch.full((R, 65), SENTINEL_I, device=DEV, dtype=torch.int32)
    dist = torch.full((R, 65), SENTINEL_F, device=DEV)
    nb = nearest_workspace_bytes(R, V, d, k)
    assert nb > 0
    ws = torch.full((max(nb, 1 << 20) // 8,), SENTINEL_I, device=DEV, dtype=torch.int64)
    A, U = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
    cases = [
        ("k = 0", dict(k=0), A), ("k > V", dict(V=2, k=3), A), ("k = 65", dict(k=65), U), ("d = 6", dict(d=6), A),
        ("d = 1028", dict(d=1028), A), ("R = 0", dict(R=0), A), ("null q", dict(q=None), A), ("null table", dict(e=None), A),
        ("null idx", dict(idx=None), A), ("null dist", dict(dist=None), A), ("null workspace", dict(ws=None), A),
        ("workspace one byte short", dict(ws_bytes=nb - 1), A),
    ]
    for what, change, code in cases:
        a = dict(q=q, e=e, R=R, V=V, d=d, k=k, idx=idx, dist=dist, ws=ws, ws_bytes=nb)
        a.update(change)
        assert _raw_call(**a) == code, what
        assert _lib.last_error(None), what
    out = C.c_int64(-1)
    assert _lib.lib.mvlpt_nearest_workspace_bytes(R, V, d, 65, None, C.byref(out)) == U and out.value == -1
    assert _lib.lib.mvlpt_nearest_workspace_bytes(R, V, d, k, None, None) == A
    torch.cuda.synchronize()
    assert bool((idx == SENTINEL_I).all()) and bool((dist == SENTINEL_F).all()) and bool((ws == SENTINEL_I).all())
    assert _raw_call(q=q[:, :d].contiguous(), e=e[:, :d].contiguous(), R=R, V=V, d=d, k=k, idx=idx, dist=dist, ws=ws, ws_bytes=nb) == 0
    torch.cuda.synchronize()
    # the same arguments unchanged are accepted; all-zero inputs: every distance ties at 0, so tokens 0 .. k-1 by index in every row
    assert idx.view(-1)[:R * k].cpu().tolist() == list(range(k)) * R and bool((dist.view(-1)[:R * k] == 0).all())
    with pytest.raises(ValueError, match="MVLPT_NEAREST_MAX_K"):
        from mvlpt_amd.interpret import nearest_words
        nearest_words(None, torch.zeros(1, d), 65)


def test_header_constants():
    from mvlpt_amd import _lib
    assert (_lib.NEAREST_MAX_K, _lib.NEAREST_MAX_ROWS) == (64, 65535 * 8)


# ------------------------------------------------------------------------------------------------ engine level
def tiny_sd(seed=1):
    from mvlpt_amd.weights import ARCHS, make_state_dict
    return make_state_dict(ARCHS["tiny"], seed, include_token_embedding=True)


def test_nearest_tokens_before_the_table_is_loaded_is_a_state_error():
    from mvlpt_amd import _lib
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    eng = Engine.from_state_dict(tiny_sd(), device=DEV, arch=ARCHS["tiny"])
    q = torch.zeros(2, 128, device=DEV)
    idx = torch.full((2, 3), SENTINEL_I, device=DEV, dtype=torch.int32)
    dist = torch.full((2, 3), SENTINEL_F, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert _lib.lib.mvlpt_nearest_tokens(eng.h, p(q), 2, 3, p(idx), p(dist), None) == _lib.ERR_STATE
    assert "not loaded" in _lib.last_error(eng.h)
    with pytest.raises(RuntimeError, match="not loaded"):
        eng.nearest_tokens(q, 3)                                  # no loader attached: the library's own refusal
    torch.cuda.synchronize()
    assert bool((idx == SENTINEL_I).all()) and bool((dist == SENTINEL_F).all())
    eng.close()


@pytest.fixture(scope="module")
def planted_clip():
    """FrozenCLIP of the tiny arch whose token table is the LARGE_R planted table (vocab 4097, width 128)."""
    from mvlpt_amd.model import FrozenCLIP
    V, d, R, k = LARGE_R
    assert d == 128
    _, E, _, _ = N.inputs(len(PLANTED), V, d, R, k)
    sd = tiny_sd()
    sd["token_embedding.weight"] = torch.from_numpy(E.copy())
    return FrozenCLIP(sd, device=DEV)


def test_engine_chunks_rows_and_agrees_with_the_kernel_entry_bit_for_bit(planted_clip):
    V, d, R, k = LARGE_R
    eng = planted_clip.engine
    calls = []

    def via_engine(Q, E, k_):
        idx, dist = eng.nearest_tokens(torch.tensor(Q).to(DEV), k_, max_rows=128)      # 300 rows: chunks of 128, 128, 44
        torch.cuda.synchronize()
        assert idx.dtype == torch.int64 and dist.dtype == torch.float32
        calls.append((idx.cpu().numpy(), dist.cpu().numpy()))
        return calls[-1]

    check_planted(len(PLANTED), V, d, R, k, via_engine)
    assert planted_clip._token_embedding_loaded                   # uploaded on first use, by encode_text's own loader
    Q, E, _, _ = N.inputs(len(PLANTED), V, d, R, k)
    idx, dist = run(Q, E, k)
    assert np.array_equal(calls[0][0], idx) and calls[0][1].tobytes() == dist.tobytes()
    whole = eng.nearest_tokens(torch.tensor(Q).to(DEV), k)
    assert np.array_equal(whole[0].cpu().numpy(), idx) and whole[1].cpu().numpy().tobytes() == dist.tobytes()
    with pytest.raises(ValueError, match="MVLPT_NEAREST_MAX_K"):
        eng.nearest_tokens(torch.tensor(Q).to(DEV), 65)


def test_golden_fixture_indices_and_distances():
    from mvlpt_amd.interpret import format_lines, nearest_words
    from mvlpt_amd.model import FrozenCLIP
    fix = np.load(N.GOLDEN)
    sd = tiny_sd(int(fix["table_seed"]))
    sd["token_embedding.weight"] = torch.from_numpy(N.golden_table(fix))
    clip = FrozenCLIP(sd, device=DEV)
    k, d = int(fix["topk"]), int(fix["width"])
    idx, dist = clip.engine.nearest_tokens(torch.from_numpy(fix["queries"]).to(DEV), k)
    assert np.array_equal(idx.cpu().numpy(), fix["out_indices"])
    N.assert_dist_inside(dist.cpu().numpy(), fix["out_distances"], d)
    rows = nearest_words(clip, torch.from_numpy(fix["queries"]), k)
    assert [[w for w, _ in row] for row in rows] == fix["out_words"].tolist()
    assert format_lines(rows) == fix["out_lines"].tolist()


# ------------------------------------------------------------------------------------------------ trainers on the live model
def _replant(clip, queries, k, seed):
    """Plant k + 1 separated neighbours of every query row into a copy of the clip's token table, upload it, and return the float64
    oracle's words per row."""
    E = clip._token_table().detach().cpu().float().numpy().copy()
    Q = queries.detach().cpu().float().reshape(-1, E.shape[1]).numpy()
    ids = N.plant(E, Q, k, np.random.default_rng(seed))
    want = N.assert_separated(N.dist64(Q, E), ids, k, E.shape[1])
    clip.engine.load_token_embedding(torch.from_numpy(E))
    clip._token_embedding_loaded = True
    dec = clip.tokenizer.decoder
    return [[dec[i] for i in row] for row in want.tolist()]


def _words(rows):
    return [[w for w, _ in row] for row in rows]


def _mvlpt(tmp_path, *, coop=0, vpt=0, csc=False, cocoop=0, classes=3, dropout=0.0):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.trainer import MVLPT, SyntheticDataManager
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.DATASET.COOP = True
    T = cfg.TRAINER.MVLPT
    T.COOP.N_CTX, T.COOP.CSC, T.VPT.N_CTX, T.COCOOP.N_CTX, T.PROJECT_DIM = coop, csc, vpt, cocoop, 64
    T.VPT.DROPOUT = dropout
    dm = SyntheticDataManager(cfg, classes, 1, device="cuda", seed=3)
    return MVLPT(cfg, dm=dm, clip_state_dict=tiny_sd(9))


@pytest.mark.parametrize("kind", ["coop", "csc", "upt"])
def test_interpret_prompt_returns_the_oracles_words(tmp_path, kind):
    torch.manual_seed(11)
    tr = _mvlpt(tmp_path, coop=4, vpt=2 if kind == "upt" else 0, csc=kind == "csc")
    pl, clip, k = tr.model.prompt_learner, tr.model.clip_model, 3
    queries = [pl.ctx.detach().reshape(-1, 128)]
    if kind == "upt":
        with torch.no_grad():
            queries.append(pl.forward_mvlpt_proj(tr.model.dtype)[0].reshape(-1, 128))
    want = _replant(clip, torch.cat(queries), k, seed=21)
    got = tr.interpret_prompt(topk=k)
    n = pl.ctx.numel() // 128
    if kind == "csc":
        assert list(got) == ["ctx"] and list(got["ctx"]) == [f"class {c}" for c in range(3)]
        flat = [row for c in got["ctx"].values() for row in c]
        assert len(flat) == 3 * 4
    else:
        flat = got["ctx"]
        assert len(flat) == 4
    assert _words(flat) == want[:n]
    if kind == "upt":
        assert list(got) == ["ctx", "ctx (projected)"]
        assert _words(got["ctx (projected)"]) == want[n:]
    else:
        assert "ctx (projected)" not in got
        with pytest.raises(RuntimeError, match="image-conditioned"):
            tr.interpret_images(torch.zeros(1, 3, 32, 32))


def test_interpret_images_on_the_cocoop_models(tmp_path):
    from mvlpt_amd.cocoop import CustomCLIP
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.model import FrozenCLIP
    torch.manual_seed(12)
    images = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    k = 3
    # trainers/cocoop.py's CoCoOp
    cfg = get_cfg_default()
    cfg.TRAINER.COCOOP.N_CTX, cfg.INPUT.SIZE = 4, (32, 32)
    model = CustomCLIP(cfg, ["dog", "cat", "sea horse"], FrozenCLIP(tiny_sd(9), device=DEV)).to(DEV)
    model.prompt_learner.eval()
    with torch.no_grad():
        model.prompt_learner.meta_net.linear2.bias.normal_(0, 0.02)       # contexts that differ from image to image AND from ctx
    ctxs = model.image_contexts(images)
    assert ctxs.shape == (3, 4, 128) and not torch.equal(ctxs[0], ctxs[1])
    want = _replant(model.clip_model, ctxs, k, seed=22)
    got = model.interpret_images(images, k)
    assert len(got) == 3 and all(len(per_image) == 4 for per_image in got)
    assert [_words(per_image) for per_image in got] == [want[4 * b:4 * b + 4] for b in range(3)]
    # the MVLPT trainer's COCOOP.N_CTX != 0 route, with visual prompts in the image tower
    tr = _mvlpt(tmp_path, vpt=2, cocoop=4)
    tr.model.prompt_learner.eval()
    ctxs = tr.model.image_contexts(images)
    want = _replant(tr.model.clip_model, torch.cat([tr.model.prompt_learner.cocoop_ctx.detach(), ctxs.reshape(-1, 128)]), k, seed=23)
    got = tr.interpret_images(images, k)
    assert [_words(per_image) for per_image in got] == [want[4 + 4 * b:8 + 4 * b] for b in range(3)]
    static = tr.interpret_prompt(topk=k)
    assert list(static) == ["cocoop_ctx"] and _words(static["cocoop_ctx"]) == want[:4]


def test_image_contexts_is_an_evaluation_forward(tmp_path):
    """With VPT dropout and the model in train mode: no mask is drawn (the RNG streams do not move), the contexts are those of eval
    mode, the mode is restored, and the backward of a forward from before the call is refused as stale instead of reading the
    activations the call replaced."""
    torch.manual_seed(13)
    tr = _mvlpt(tmp_path, vpt=2, cocoop=4, dropout=0.5)
    model, pl = tr.model, tr.model.prompt_learner
    images = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    pl.eval()
    want = model.image_contexts(images)
    pl.train()
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    got = model.image_contexts(images)
    assert torch.equal(got, want) and pl.training
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(DEV), gpu_rng)
    logits = model(images)
    model.image_contexts(images)
    with pytest.raises(RuntimeError, match="stale forward"):
        logits.sum().backward()
    pl.zero_grad(set_to_none=True)
    model(images).sum().backward()                                # the next forward / backward pair is untouched
    torch.cuda.synchronize()
    assert pl.cocoop_ctx.grad is not None and bool(torch.isfinite(pl.cocoop_ctx.grad).all())
