"""The zero-shot glue kernels at kernel level (-m gpu): embed_tokens bit for bit against torch, ensemble_features inside the derived
per-element bound of tests/zs_ref.py, and the host-side argument checks of mvlpt_text_encode_tokens."""
import numpy as np
import pytest
import torch

from tests import zs_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VOCAB, LD, MIN_L = 97, 77, 3
SENTINEL = -12345.0


# ------------------------------------------------------------------------------------------------ embed_tokens
def test_minimum_length_is_the_header_constant():
    from mvlpt_amd import _lib
    assert _lib.TEXT_MIN_L == MIN_L


@pytest.mark.parametrize("d", [128, 512, 768])
@pytest.mark.parametrize("L", [MIN_L, 7, 77])
@pytest.mark.parametrize("S", [1, 5])
def test_embed_tokens_bit_exact(S, L, d):
    from mvlpt_amd.engine import op_embed_tokens
    g = torch.Generator().manual_seed(1000 * S + 10 * L + d)
    emb, pos = torch.randn(VOCAB, d, generator=g), torch.randn(LD, d, generator=g)
    ids = torch.randint(0, VOCAB, (S, LD), generator=g, dtype=torch.int32)
    ids[0, 0], ids[-1, L - 1], ids[0, 1] = 0, VOCAB - 1, ids[0, 2]          # both ends of the table and a repeat
    ids[:, L:] = 10 ** 9                                                      # never read: out-of-range on purpose
    if L + 1 < LD:
        ids[:, L + 1] = -1
    want = emb[ids[:, :L].long()] + pos[:L]
    assert torch.equal(want, zs_ref.embed_ref64(emb, pos, ids, L).float())   # one fp32 add is exactly rounded
    n = S * L * d
    runs = []
    for _ in range(2):
        buf = torch.full((n + 1024,), SENTINEL, device=DEV)
        op_embed_tokens(emb.to(DEV), pos.to(DEV), ids.to(DEV), L, out=buf)
        torch.cuda.synchronize()
        got = buf.cpu()
        assert bool((got[n:] == SENTINEL).all()), "wrote behind the output"
        runs.append(got[:n].view(S, L, d))
    assert torch.equal(runs[0], want)
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ ensemble_features
@pytest.mark.parametrize("e", [128, 512, 768])
@pytest.mark.parametrize("C", [1, 5, 130])
@pytest.mark.parametrize("T", [1, 2, 8, 81])
def test_ensemble_features_inside_the_derived_bound(T, C, e):
    from mvlpt_amd.engine import op_ensemble_features, op_normalize_rows
    f = zs_ref.ensemble_inputs(T, C, e)
    fd = f.to(DEV)
    got = op_ensemble_features(fd)
    again = op_ensemble_features(fd)
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    err = (got.cpu().double() - zs_ref.ensemble_ref64(f)).abs()
    bound = zs_ref.ensemble_bound(f)
    print(f"T {T} C {C} e {e}: max err {float(err.max()):.3e} max bound {float(bound.max()):.3e} worst ratio {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    if T == 1:
        xn, _ = op_normalize_rows(fd[0])
        assert torch.equal(got, xn), "one template is the head's row normalisation, bit for bit"


def test_ensemble_refuses_an_embed_dim_it_cannot_hold():
    from mvlpt_amd.engine import op_ensemble_features
    with pytest.raises(RuntimeError):
        op_ensemble_features(torch.zeros(2, 3, 1028, device=DEV))


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope="module")
def tiny_clip():
    from mvlpt_amd.model import FrozenCLIP
    from mvlpt_amd.weights import ARCHS, make_state_dict
    return FrozenCLIP(make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True), device=DEV)


def _row(eot_at, vocab, ld=77):
    ids = np.zeros((1, ld), dtype=np.int32)
    ids[0, 0] = vocab - 2
    ids[0, 1:eot_at] = 5
    ids[0, eot_at] = vocab - 1
    return ids


def test_encode_tokens_refuses_bad_tables_on_the_host(tiny_clip):
    eng, vocab = tiny_clip.engine, tiny_clip.arch.vocab_size
    good = _row(6, vocab)
    with pytest.raises(RuntimeError, match="not loaded"):
        eng.text_encode_tokens(good, 8)                          # no token embedding yet
    eng.load_token_embedding(tiny_clip._token_table())
    ref = eng.text_encode_tokens(good, 8).cpu()
    for bad_id in (-1, vocab):
        ids = good.copy()
        ids[0, 3] = bad_id
        if bad_id == vocab:
            ids[0, 6] = 5                                        # (the row maximum is the bad id itself)
        with pytest.raises(RuntimeError, match=r"outside \[0, vocab\)|EOT"):
            eng.text_encode_tokens(ids, 8)
    ids = good.copy()
    ids[0, 3] = -1
    with pytest.raises(RuntimeError, match=r"outside \[0, vocab\)"):
        eng.text_encode_tokens(ids, 8)
    with pytest.raises(RuntimeError, match="EOT"):
        eng.text_encode_tokens(good, 6)                          # EOT at L
    with pytest.raises(RuntimeError, match="EOT"):
        eng.text_encode_tokens(_row(40, vocab), 8)               # EOT beyond L
    with pytest.raises(RuntimeError, match="context_length"):
        eng.text_encode_tokens(_row(6, vocab, ld=80), 78)
    with pytest.raises(RuntimeError, match="MVLPT_TEXT_MIN_L"):
        eng.text_encode_tokens(_row(1, vocab), 2)
    # an id outside the table behind column L is never read, and the engine still computes what it computed before the refusals
    ids = good.copy()
    ids[0, 9:] = -7
    torch.cuda.synchronize()
    assert torch.equal(eng.text_encode_tokens(ids, 8).cpu(), ref)
