"""Host side of prompt interpretation (no GPU): mvlpt_amd.interpret over a stand-in engine whose nearest_tokens is float64 numpy
(Float64Engine below), on checkpoints written in the Dassl dict form, and against tests/golden/interpret.npz (expected
decoder strings and printed lines from the reference's tokenizer and stock torch.cdist / torch.argsort)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import nearest_ref as N


class Float64Engine:
    """Stand-in for mvlpt_amd.engine.Engine on the host: nearest_tokens over a numpy table in float64, ties by index."""

    def __init__(self, table: np.ndarray):
        self.table = np.asarray(table, dtype=np.float32)
        self.calls = []

    def nearest_tokens(self, q, k):
        qn = q.detach().cpu().numpy().astype(np.float32)
        self.calls.append(tuple(qn.shape))
        D = N.dist64(qn, self.table)
        idx = N.topk64(D, k)
        return torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(np.take_along_axis(D, idx, axis=1).astype(np.float32))


@pytest.fixture(scope="module")
def fix():
    return np.load(N.GOLDEN)


@pytest.fixture(scope="module")
def clip(fix):
    """FrozenCLIP's interpretation surface on the host: the planted fixture table behind a float64 engine, the shipped tokenizer."""
    from mvlpt_amd.model import default_tokenizer
    return SimpleNamespace(engine=Float64Engine(N.golden_table(fix)), tokenizer=default_tokenizer())


def _save(tmp_path, state_dict, name="model.pth.tar-50"):
    path = tmp_path / "prompt_learner" / name
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save({"state_dict": state_dict, "epoch": 50, "optimizer": None, "scheduler": None, "val_result": 0.0}, path)
    return torch.load(path, map_location="cpu")


def _words(rows):
    return [[w for w, _ in row] for row in rows]


def test_decoder_matches_the_reference_tokenizer(fix, clip):
    dec = clip.tokenizer.decoder
    assert [[dec[i] for i in row] for row in fix["out_indices"].tolist()] == fix["out_words"].tolist()
    assert len(dec) == int(fix["vocab"])


def test_the_stand_in_engine_reproduces_the_fixture(fix, clip):
    idx, dist = clip.engine.nearest_tokens(torch.from_numpy(fix["queries"]), int(fix["topk"]))
    assert np.array_equal(idx.numpy(), fix["out_indices"])
    N.assert_dist_inside(dist.numpy(), fix["out_distances"], int(fix["width"]))


def test_generic_checkpoint_prints_the_reference_lines(tmp_path, fix, clip):
    from mvlpt_amd.interpret import format_lines, interpret_state_dict
    q = torch.from_numpy(fix["queries"])
    ck = _save(tmp_path, {"ctx": q, "token_prefix": torch.zeros(2, 1, 128), "token_suffix": torch.zeros(2, 70, 128)})
    got = interpret_state_dict(ck, clip, int(fix["topk"]))                         # the whole Dassl dict is accepted
    assert list(got) == ["ctx"]
    assert _words(got["ctx"]) == fix["out_words"].tolist()
    assert format_lines(got["ctx"]) == fix["out_lines"].tolist()
    assert format_lines(got) == ["ctx:"] + fix["out_lines"].tolist()
    assert got == interpret_state_dict(ck["state_dict"], clip, int(fix["topk"]))   # ... and so is the state dict alone
    for row, want in zip(got["ctx"], fix["out_distances"]):
        assert all(isinstance(w, str) and isinstance(x, float) for w, x in row)
        N.assert_dist_inside(np.array([x for _, x in row]), want, int(fix["width"]))


def test_csc_checkpoint_gives_one_list_per_class(tmp_path, fix, clip):
    from mvlpt_amd.interpret import format_lines, interpret_state_dict
    q = torch.from_numpy(fix["queries"])
    ctx = torch.stack([q, q.flip(0)])                                              # [2 classes, 3, width]
    ck = _save(tmp_path, {"ctx": ctx, "token_prefix": torch.zeros(2, 1, 128)})
    calls = len(clip.engine.calls)
    got = interpret_state_dict(ck, clip, 2, classnames=["dog", "sea horse"])
    assert clip.engine.calls[calls:] == [(6, 128)]                                 # every class in ONE nearest-token call
    want = [row[:2] for row in fix["out_words"].tolist()]
    assert list(got["ctx"]) == ["dog", "sea horse"]
    assert _words(got["ctx"]["dog"]) == want and _words(got["ctx"]["sea horse"]) == want[::-1]
    lines = format_lines(got)
    assert lines[0] == "ctx / dog:" and lines[4] == "ctx / sea horse:" and len(lines) == 8
    assert lines[1].startswith("1: ['") and lines[5].startswith("1: ['")
    assert list(interpret_state_dict(ck, clip, 2)["ctx"]) == ["class 0", "class 1"]
    with pytest.raises(ValueError, match="2 classes but 3 class names"):
        interpret_state_dict(ck, clip, 2, classnames=["a", "b", "c"])


def test_cocoop_ctx_checkpoint(tmp_path, fix, clip):
    from mvlpt_amd.interpret import interpret_state_dict
    q = torch.from_numpy(fix["queries"])
    ck = _save(tmp_path, {"cocoop_ctx": q[1:], "meta_net.linear1.weight": torch.zeros(8, 128), "token_suffix": torch.zeros(2, 70, 128)})
    got = interpret_state_dict(ck, clip, 4)
    assert list(got) == ["cocoop_ctx"]
    assert _words(got["cocoop_ctx"]) == [row[:4] for row in fix["out_words"].tolist()[1:]]


def test_nearest_words_restores_the_leading_dimensions(fix, clip):
    from mvlpt_amd.interpret import nearest_words
    q = torch.from_numpy(fix["queries"])
    want = [row[:1] for row in fix["out_words"].tolist()]
    got = nearest_words(clip, torch.stack([q, q]).reshape(2, 1, 3, 128), 1)
    assert len(got) == 2 and len(got[0]) == 1 and _words(got[0][0]) == want and _words(got[1][0]) == want
    assert [w for w, _ in nearest_words(clip, q[2], 1)] == want[2]                 # a single vector: its own list
    other = SimpleNamespace(decoder=[str(i) for i in range(int(fix["vocab"]))])
    assert _words(nearest_words(clip, q, 1, tokenizer=other)) == [[str(r[0])] for r in fix["out_indices"].tolist()]


def test_error_messages(tmp_path, fix, clip):
    from mvlpt_amd import _lib
    from mvlpt_amd.interpret import interpret_state_dict, nearest_words
    ck = _save(tmp_path, {"vpt_embeddings": torch.zeros(1, 2, 128), "token_prefix": torch.zeros(2, 1, 128)})
    with pytest.raises(ValueError, match=r"no context tensor \(ctx / cocoop_ctx\).*token_prefix, vpt_embeddings"):
        interpret_state_dict(ck, clip, 5)
    q = torch.from_numpy(fix["queries"])
    assert _lib.NEAREST_MAX_K == 64
    for bad in (65, 0):
        with pytest.raises(ValueError, match=rf"topk must lie in \[1, 64\] \(MVLPT_NEAREST_MAX_K\), got {bad}"):
            interpret_state_dict({"ctx": q}, clip, bad)
        with pytest.raises(ValueError, match="MVLPT_NEAREST_MAX_K"):
            nearest_words(clip, q, bad)
    with pytest.raises(ValueError, match=r"must be \[n_ctx, width\] or \[n_cls, n_ctx, width\]"):
        interpret_state_dict({"ctx": q.reshape(1, 1, 3, 128)}, clip, 5)


def _load_tool():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("interpret_prompt_tool", os.path.join(root, "tools", "interpret_prompt.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_prints_the_reference_lines(tmp_path, fix, monkeypatch, capsys):
    """tools/interpret_prompt.py end to end on the host, on both table sources: only the device copy of the table (TokenTable) is
    replaced by the float64 stand-in."""
    from mvlpt_amd.model import default_tokenizer
    tool = _load_tool()
    tables = []

    def host_table(table):
        tables.append(table)
        return SimpleNamespace(engine=Float64Engine(table.numpy()), tokenizer=default_tokenizer())

    monkeypatch.setattr(tool, "TokenTable", host_table)
    k = int(fix["topk"])
    ckpt = tmp_path / "model.pth.tar-50"
    torch.save({"state_dict": {"ctx": torch.from_numpy(fix["queries"]), "token_prefix": torch.zeros(2, 1, 128)}, "epoch": 50}, ckpt)
    # --weights: a CLIP state dict whose token table is the fixture's planted one
    planted = torch.from_numpy(N.golden_table(fix))
    weights = tmp_path / "clip_state_dict.pt"
    torch.save({"token_embedding.weight": planted, "logit_scale": torch.tensor(4.6)}, weights)
    assert tool.main([str(ckpt), str(k), "--weights", str(weights)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == f"Return the top-{k} matched words"
    assert out[1] == "Size of token embedding: torch.Size([49408, 128])" and out[2] == "Size of context: torch.Size([3, 128])"
    assert out[3:] == fix["out_lines"].tolist()
    assert torch.equal(tables[-1], planted)
    # no weights: the seeded table FrozenCLIP falls back to, announced on the first line
    assert tool.main([str(ckpt), "2", "--backbone", "tiny"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert "seeded" in out[0] and out[1] == "Return the top-2 matched words" and len(out) == 4 + 3
    from mvlpt_amd.weights import _randn
    assert torch.equal(tables[-1], _randn("token_embedding.weight", 0, (49408, 128), 0.02))
    for bad in (["missing.pth", "5"], [str(ckpt), "5", "--weights", str(tmp_path / "none.pt")], [str(ckpt), "5", "--backbone", "RN50"],
                [str(ckpt), "5", "--weights", str(ckpt)]):
        with pytest.raises(SystemExit):
            tool.main(bad)
