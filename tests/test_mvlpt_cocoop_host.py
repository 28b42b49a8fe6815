"""MVLPT's CoCoOp route (mvlpt_amd.mvlpt_cocoop) host side, CPU only: the prompt learner's checkpoint keys, buffers and integer
tables against fixtures generated through the REAL reference (tools/make_mvlpt_cocoop_golden.py), the class-range tables and the
chunking, and which model class MVLPT.build_model picks."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.golden_util import GOLDEN, load_npz, t

TINY_CASES = ["tiny_mvlpt_cocoop", "tiny_mvlpt_cocoop_mask", "tiny_mvlpt_cocoop_mask_soft", "tiny_mvlpt_cocoop_vpt",
              "tiny_mvlpt_cocoop_ctxinit", "tiny_mvlpt_cocoop_cut"]
ALL_CASES = TINY_CASES + ["full_vitb16_mvlpt_cocoop_mask"]


def mvlpt_cocoop_cfg(case, image_size):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    T = cfg.TRAINER.MVLPT
    T.COCOOP.N_CTX, T.COCOOP.CTX_INIT, T.COCOOP.PREC = int(case["meta_n_ctx_cfg"]), str(case["meta_ctx_init"]), "fp32"
    T.VPT.N_CTX, T.VPT.DEEP = int(case["meta_vpt_n_ctx"]), bool(int(case["meta_vpt_deep"])) or not int(case["meta_vpt_n_ctx"])
    cfg.TRAINER.CUT_CONTEXTLEN = bool(int(case["meta_cut"]))
    cfg.INPUT.SIZE = (image_size, image_size)
    cfg.DATASET.MULTITASK = cfg.DATASET.MULTITASK_LABEL_PERTASK = "task" in case
    return cfg


def case_dm(case):
    """Data-manager stand-in for CustomCLIP's per-task tables (trainers/mvlpt.py:527-538), or None without the mask."""
    if "task" not in case:
        return None
    counts = case["task_counts"].tolist()
    names = [f"task{i}" for i in range(len(counts))]
    return SimpleNamespace(_num_classes=int(case["out_logits"].shape[1]), _task_names=names,
                           _labelmap={n: list(range(c)) for n, c in zip(names, counts)})


def tiny_sd_with_tokens():
    from mvlpt_amd.weights import ARCHS, make_state_dict
    return make_state_dict(ARCHS["tiny"], 1, include_token_embedding=True)      # oracle/make_golden.py TINY_SEED: tiny_clip.npz


def host_prompt_learner(case, sd, pretokenized=False):
    """The prompt learner built on the oracle-backed frozen CLIP, with the real BPE tokenizer and the fixture's class names."""
    from mvlpt_amd.model import PretokenizedPrompts, default_tokenizer
    from mvlpt_amd.mvlpt_cocoop import MultitaskVLPromptLearner
    from mvlpt_amd.weights import ARCHS
    from tests.fake_engine import OracleFrozenCLIP
    arch = ARCHS["tiny"]
    clip = OracleFrozenCLIP(sd, arch)
    clip._emb = sd["token_embedding.weight"].float()
    clip.tokenizer = default_tokenizer()
    torch.manual_seed(int(case["case_seed"]))
    pre = PretokenizedPrompts(t(case["tokenized_prompts"]), case["name_lens"].tolist()) if pretokenized else None
    return MultitaskVLPromptLearner(mvlpt_cocoop_cfg(case, arch.image_resolution), [str(n) for n in case["classnames"]], clip, pre)


@pytest.mark.parametrize("key,name", [("state_dict", "tiny_mvlpt_cocoop"), ("state_dict_vpt", "tiny_mvlpt_cocoop_vpt")])
def test_state_dict_keys_and_shapes_match_reference(key, name):
    ref = json.load(open(os.path.join(GOLDEN, "ref_mvlpt_cocoop_prompt_learner.json")))[key]
    pl = host_prompt_learner(load_npz(name), tiny_sd_with_tokens())
    own = {k: list(v.shape) for k, v in pl.state_dict().items()}
    assert list(own) == list(ref), "checkpoint keys (and their order) must be the reference's"
    assert own == ref
    assert all(p.dtype == torch.float32 for p in pl.parameters())                 # fp32 masters


@pytest.mark.parametrize("name", TINY_CASES)
def test_buffers_layout_and_tokens_bit_exact_and_strict_load(name):
    case = load_npz(name)
    pl = host_prompt_learner(case, tiny_sd_with_tokens())
    assert np.array_equal(pl.tokenized_prompts.numpy(), case["tokenized_prompts"])
    assert pl.name_lens == case["name_lens"].tolist()
    assert np.array_equal(pl.token_prefix.numpy(), case["token_prefix"])
    assert np.array_equal(pl.token_suffix.numpy(), case["token_suffix"])
    assert np.array_equal(pl.layout.numpy(), case["layout"]), "construct_prompts' layout must be bit-exact"
    assert np.array_equal(pl.eot.numpy().astype(np.int64), case["eot"])
    assert pl.cocoop_n_ctx == int(case["meta_n_ctx"]) and pl.coop_n_ctx == 0
    state = {k[len("param_"):]: t(v) for k, v in case.items() if k.startswith("param_")}
    state["token_prefix"], state["token_suffix"] = t(case["token_prefix"]), t(case["token_suffix"])
    pl.load_state_dict(state, strict=True)


def test_ctx_init_and_random_init_follow_the_reference():
    case = load_npz("tiny_mvlpt_cocoop_ctxinit")
    pl = host_prompt_learner(case, tiny_sd_with_tokens())
    assert pl.cocoop_n_ctx == 4 == int(case["meta_n_ctx"]) != int(case["meta_n_ctx_cfg"])
    assert np.array_equal(pl.cocoop_ctx.detach().numpy(), case["param_cocoop_ctx"]), "ctx must start as the words' token embeddings"
    case = load_npz("tiny_mvlpt_cocoop")
    pl = host_prompt_learner(case, tiny_sd_with_tokens())           # same seed, same draw order (cocoop_ctx, then meta_net)
    assert np.array_equal(pl.cocoop_ctx.detach().numpy(), case["param_cocoop_ctx"])
    assert np.array_equal(pl.meta_net.linear1.weight.detach().numpy(), case["param_meta_net.linear1.weight"])


def test_full_fixture_tables():
    from mvlpt_amd.model import build_prompt_layout
    case = load_npz("full_vitb16_mvlpt_cocoop_mask")
    n, L = int(case["meta_n_ctx"]), case["tokenized_prompts"].shape[1]
    assert np.array_equal(build_prompt_layout(case["name_lens"].tolist(), n, L, "end").numpy(), case["layout"])
    assert np.array_equal(case["tokenized_prompts"].argmax(-1), case["eot"])


def test_class_ranges_and_chunks():
    from mvlpt_amd.per_image_text import chunk_bounds, class_ranges
    start, end = torch.arange(6), torch.arange(6)
    start[:3], end[:3] = torch.tensor([0, 2, 3]), torch.tensor([2, 3, 6])          # task_counts [2, 1, 3], sized num_classes
    for task, lo, hi in [([0, 1, 2], [0, 2, 3], [2, 3, 6]),                         # ordered
                         ([2, 2, 2, 0], [3, 3, 3, 0], [6, 6, 6, 2]),                # repeated
                         ([2, 0, 1, 2, 0, 2], [3, 0, 2, 3, 0, 3], [6, 2, 3, 6, 2, 6])]:   # out of order
        for tk in (task, torch.tensor(task), np.array(task)):
            assert class_ranges(tk, start, end, len(task), 6) == (lo, hi)
        widths = [b - a for a, b in zip(lo, hi)]
        S = sum(widths)
        assert chunk_bounds(widths, lambda s: True) == [(0, len(task), S)]
        for cap in (1, 3, 4, 5):
            ch = chunk_bounds(widths, lambda s: s <= cap)
            assert ch[0][0] == 0 and ch[-1][1] == len(task) and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
            assert all(s == sum(widths[g0:g1]) for g0, g1, s in ch) and sum(c[2] for c in ch) == S
            assert all(s <= cap or g1 - g0 == 1 for g0, g1, s in ch), "only a single image may exceed the budget"
            # greedy: the next image would not have fitted
            assert all(a[2] + widths[b[0]] > cap for a, b in zip(ch, ch[1:]))
    assert class_ranges(None, None, None, 3, 5) == ([0, 0, 0], [5, 5, 5])
    assert chunk_bounds([3, 0, 0, 3, 0], lambda s: s <= 3) == [(0, 3, 3), (3, 5, 3)]    # empty ranges ride along
    assert chunk_bounds([0, 0], lambda s: False) == [(0, 2, 0)]
    with pytest.raises(ValueError):
        class_ranges([0, 1], start, end, 3, 6)


def test_coop_together_with_cocoop_is_refused():
    case = dict(load_npz("tiny_mvlpt_cocoop"))
    from mvlpt_amd.mvlpt_cocoop import MultitaskVLPromptLearner
    from mvlpt_amd.weights import ARCHS
    from tests.fake_engine import OracleFrozenCLIP
    cfg = mvlpt_cocoop_cfg(case, 32)
    cfg.TRAINER.MVLPT.COOP.N_CTX = 4
    with pytest.raises(NotImplementedError, match="COOP.N_CTX"):
        MultitaskVLPromptLearner(cfg, ["a", "b"], OracleFrozenCLIP(tiny_sd_with_tokens(), ARCHS["tiny"]))


def test_build_model_picks_the_route_iff_cocoop_n_ctx(monkeypatch):
    """MVLPT.build_model's choice, without a GPU: the model classes are replaced by recorders."""
    import mvlpt_amd.mvlpt_cocoop as mc
    import mvlpt_amd.trainer as tr
    picked = []

    class _Stop(Exception):
        pass

    def recorder(tag):
        def ctor(*a, **k):
            picked.append(tag)
            raise _Stop()
        return ctor
    monkeypatch.setattr(tr, "CustomCLIP", recorder("model"))
    monkeypatch.setattr(mc, "CustomCLIP", recorder("mvlpt_cocoop"))
    monkeypatch.setattr(tr, "FrozenCLIP", lambda *a, **k: None)
    from mvlpt_amd.config import get_cfg_default
    for n_ctx, want in ((0, "model"), (4, "mvlpt_cocoop"), (16, "mvlpt_cocoop")):
        cfg = get_cfg_default()
        cfg.MODEL.BACKBONE.NAME = "tiny"
        cfg.INPUT.SIZE = (32, 32)
        cfg.TRAINER.MVLPT.COOP.N_CTX = 0 if n_ctx else 4
        cfg.TRAINER.MVLPT.COCOOP.N_CTX = n_ctx
        self = SimpleNamespace(cfg=cfg, dm=SimpleNamespace(dataset=SimpleNamespace(classnames=["a", "b"]), lab2cname={0: "a", 1: "b"}),
                               _sd_arg={}, device="cpu")
        with pytest.raises(_Stop):
            tr.MVLPT.build_model(self)
        assert picked[-1] == want
