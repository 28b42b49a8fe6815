"""Tip-Adapter without a GPU: the C ABI's new symbols and caps, the config keys, the published grid, cache building on a fake engine
(epoch average, double normalisation, stable sort, key_ptr), the winner rule, the state dict, the launcher's registration and the
trainer's refusals."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import tip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


class FakeEngine:
    """The two engine calls the host logic makes, in torch on the CPU."""

    def __init__(self, counts=None, grid=None):
        self.counts, self.grid, self.search_calls = counts, grid, []

    def text_ensemble(self, feats):
        assert feats.dim() == 3
        return unit(unit(feats).mean(0))

    def tip_search(self, F, y, K, key_ptr, W, s, betas, alphas):
        self.search_calls.append((betas.clone(), alphas.clone()))
        b0 = int(np.argmin(np.abs(np.float32(self.grid[0]) - float(betas[0]))))      # where this piece sits in the whole grid
        a0 = int(np.argmin(np.abs(np.float32(self.grid[1]) - float(alphas[0]))))
        return torch.from_numpy(self.counts[b0:b0 + len(betas), a0:a0 + len(alphas)].astype(np.int32))


class FakeClip:
    @staticmethod
    def encode_image(images):
        return images.flatten(1)


def head(n_cls=5, dim=8, **kw):
    from mvlpt_amd.tip_adapter import TipAdapterHead
    g = torch.Generator().manual_seed(0)
    return TipAdapterHead(kw.pop("engine", FakeEngine()), unit(torch.randn(n_cls, dim, generator=g)), 100.0, **kw)


# ------------------------------------------------------------------------------------------------ ABI and config
def test_abi_exports_the_tip_symbols():
    from mvlpt_amd import _lib
    for name in ("mvlpt_tip_workspace_bytes", "mvlpt_op_tip_logits", "mvlpt_op_tip_train_fwd", "mvlpt_op_tip_train_bwd",
                 "mvlpt_op_tip_search"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), f"{name} is not exported by libmvlpt_hip.so"
    header = open(os.path.join(ROOT, "include", "mvlpt_hip.h")).read()
    assert f"MVLPT_TIP_MAX_NB = {_lib.TIP_MAX_NB}, MVLPT_TIP_MAX_NA = {_lib.TIP_MAX_NA}" in header
    assert f"MVLPT_TIP_LOGITS = {_lib.TIP_LOGITS}, MVLPT_TIP_TRAIN = {_lib.TIP_TRAIN}, MVLPT_TIP_SEARCH = {_lib.TIP_SEARCH}" in header
    assert _lib.TIP_MAX_CLASSES == 1 << 20 and "MVLPT_TIP_MAX_CLASSES = 1 << 20" in header
    from mvlpt_amd import tip_adapter
    assert (tip_adapter.MAX_NB, tip_adapter.MAX_NA) == (_lib.TIP_MAX_NB, _lib.TIP_MAX_NA)


def test_workspace_entry_answers_without_a_device():
    """Sizes are host arithmetic: the 1 GiB limit of the search at ImageNet size holds wherever the library loads."""
    import ctypes as C

    from mvlpt_amd import _lib
    out = C.c_int64(-1)
    for D in (512, 1024):
        assert _lib.lib.mvlpt_tip_workspace_bytes(50000, 16000, 1000, D, 200, 20, _lib.TIP_SEARCH, C.byref(out)) == 0
        assert 0 < out.value < (1 << 30)
    assert _lib.lib.mvlpt_tip_workspace_bytes(256, 16000, 1000, 1024, 0, 0, _lib.TIP_TRAIN, C.byref(out)) == 0
    assert 256 * 16000 * 4 <= out.value < (1 << 26)
    assert _lib.lib.mvlpt_tip_workspace_bytes(256, 16000, 1000, 1022, 0, 0, _lib.TIP_TRAIN, C.byref(out)) == _lib.ERR_ARG
    assert "D must be a multiple of 4" in _lib.last_error(None)
    assert _lib.lib.mvlpt_tip_workspace_bytes(8, 8, 8, 8, _lib.TIP_MAX_NB + 1, 1, _lib.TIP_SEARCH, C.byref(out)) == _lib.ERR_ARG
    # row and key counts that would overflow their rounding to whole tiles are refused, with one class too
    header = open(os.path.join(ROOT, "include", "mvlpt_hip.h")).read()
    assert _lib.TIP_MAX_ROWS == 2 ** 31 - 256 and f"MVLPT_TIP_MAX_ROWS = {_lib.TIP_MAX_ROWS}" in header
    for mode in (_lib.TIP_LOGITS, _lib.TIP_TRAIN, _lib.TIP_SEARCH):
        assert _lib.lib.mvlpt_tip_workspace_bytes(2 ** 31 - 1, 8, 1, 8, 1, 1, mode, C.byref(out)) == _lib.ERR_ARG
        assert _lib.lib.mvlpt_tip_workspace_bytes(8, _lib.TIP_MAX_ROWS + 1, 1, 8, 1, 1, mode, C.byref(out)) == _lib.ERR_ARG
    assert "MVLPT_TIP_MAX_ROWS" in _lib.last_error(None)
    assert _lib.lib.mvlpt_tip_workspace_bytes(_lib.TIP_MAX_ROWS, 8, 1, 8, 1, 1, _lib.TIP_LOGITS, C.byref(out)) == 0


def test_config_defaults():
    from mvlpt_amd.config import get_cfg_default
    T = get_cfg_default().TRAINER.TIP
    assert (T.AUGMENT_EPOCH, T.INIT_ALPHA, T.INIT_BETA, T.SEARCH_HP, T.FINETUNE, T.TRAIN_EPOCH, T.LR, T.EPS) == \
        (10, 1.0, 5.5, True, False, 20, 1e-3, 1e-4)
    assert list(T.SEARCH_SCALE) == [7.0, 3.0] and list(T.SEARCH_STEP) == [200, 20]
    cfg = get_cfg_default()
    cfg.merge_from_list(["TRAINER.TIP.FINETUNE", "True", "TRAINER.TIP.SEARCH_STEP", "[20, 5]"])
    assert cfg.TRAINER.TIP.FINETUNE is True and list(cfg.TRAINER.TIP.SEARCH_STEP) == [20, 5]


def test_grid_is_the_published_formula():
    from mvlpt_amd.tip_adapter import search_grid
    betas, alphas = search_grid()
    assert betas == [i * (7.0 - 0.1) / 200 + 0.1 for i in range(200)]
    assert alphas == [i * (3.0 - 0.1) / 20 + 0.1 for i in range(20)]
    rb, ra = R.published_grid()
    assert np.array_equal(np.asarray(betas), rb) and np.array_equal(np.asarray(alphas), ra)
    assert search_grid((1.0, 2.0), (1, 3)) == ([0.1], [0.1, 0.1 + 1.9 / 3, 0.1 + 2 * 1.9 / 3])
    with pytest.raises(ValueError):
        search_grid((7.0, 3.0), (0, 20))


def test_winner_is_the_first_strict_maximum():
    from mvlpt_amd.tip_adapter import first_maximum
    counts = np.array([[1, 5, 5], [5, 2, 5], [0, 5, 1]])
    assert first_maximum(counts) == (0, 1) == R.winner(counts)
    assert first_maximum(np.zeros((3, 2))) == (0, 0)


# ------------------------------------------------------------------------------------------------ the cache
def test_cache_is_the_normalised_epoch_mean_sorted_stably_by_class():
    h = head()
    g = torch.Generator().manual_seed(1)
    labels = [3, 0, 3, 1, 0, 4, 3]                       # class 2 owns no key
    passes = [torch.randn(7, 2, 2, 2, generator=g) * (1 + e) for e in range(3)]      # another augmentation every pass
    calls = []

    def batches_fn():
        x = passes[len(calls)]
        calls.append(1)
        return [(x[:4], torch.tensor(labels[:4])), (x[4:], torch.tensor(labels[4:]))]

    h.build_cache(FakeClip, batches_fn, augment_epochs=3)
    assert len(calls) == 3
    want = unit(torch.stack([unit(p.flatten(1)) for p in passes]).mean(0))
    order = [1, 4, 3, 0, 2, 6, 5]
    assert torch.allclose(h.keys, want[order], atol=1e-6)
    assert torch.allclose(h.keys.norm(dim=-1), torch.ones(7), atol=1e-6)
    assert h.key_labels.tolist() == [0, 0, 1, 3, 3, 3, 4]
    assert h.key_ptr.dtype == torch.int32 and h.key_ptr.tolist() == [0, 2, 3, 3, 6, 7]
    # the same from arrays: one pass
    h2 = head().from_features(passes[0].flatten(1), labels, 5)
    assert torch.allclose(h2.keys, unit(passes[0].flatten(1))[order], atol=1e-6) and torch.equal(h2.key_ptr, h.key_ptr)


def test_cache_refusals():
    h = head()
    x = torch.randn(4, 8)
    state = {"n": 0}

    def shuffled():
        state["n"] += 1
        return [(x, torch.tensor([0, 1, 2, 3] if state["n"] == 1 else [0, 1, 3, 2]))]

    with pytest.raises(ValueError, match="labels differ"):
        h.build_cache(FakeClip, shuffled, augment_epochs=2)
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        h.from_features(x, [0, 1, 2, 5])
    with pytest.raises(ValueError, match="n_cls"):
        h.from_features(x, [0, 1, 2, 3], n_cls=4)
    with pytest.raises(ValueError, match="features must be"):
        h.from_features(torch.randn(4, 12), [0, 1, 2, 3])
    with pytest.raises(ValueError):
        h.build_cache(FakeClip, lambda: [], augment_epochs=1)
    with pytest.raises(RuntimeError, match="cache is empty"):
        head().logits(x)
    with pytest.raises(RuntimeError, match="cache is empty"):
        head().state_dict()


def test_state_dict_round_trip():
    h = head(alpha=2.5, beta=0.75).from_features(torch.randn(6, 8), [4, 0, 2, 0, 4, 1])
    sd = h.state_dict()
    assert set(sd) == {"keys", "key_labels", "alpha", "beta"}
    g = head().load_state_dict(sd)
    assert torch.equal(g.keys, h.keys) and torch.equal(g.key_ptr, h.key_ptr) and torch.equal(g.key_labels, h.key_labels)
    assert (g.alpha, g.beta) == (2.5, 0.75)
    sd["keys"] += 1.0                                     # a copy: the head keeps its keys
    assert not torch.equal(sd["keys"], h.keys)
    with pytest.raises(ValueError):
        head(dim=12).load_state_dict(h.state_dict())


def test_search_sets_the_first_best_grid_point():
    from mvlpt_amd.tip_adapter import search_grid
    counts = np.zeros((200, 20), np.int64)
    counts[7, 3] = counts[7, 9] = counts[150, 0] = 11
    eng = FakeEngine(counts, search_grid())
    h = head(engine=eng).from_features(torch.randn(6, 8), [4, 0, 2, 0, 4, 1])
    beta, alpha, acc, got = h.search_hp(torch.randn(12, 8), torch.arange(12) % 5)
    betas, alphas = search_grid()
    assert len(eng.search_calls) == 1                     # the published grid is ONE call
    assert eng.search_calls[0][0].dtype == torch.float32 and len(eng.search_calls[0][0]) == 200 and len(eng.search_calls[0][1]) == 20
    assert (beta, alpha) == (betas[7], alphas[3]) == (h.beta, h.alpha)
    assert acc == pytest.approx(100.0 * 11 / 12) and np.array_equal(got, counts)
    with pytest.raises(ValueError):
        h.search_hp(torch.randn(12, 8), torch.arange(12))        # labels outside the classes


def test_a_grid_above_the_caps_is_refused():
    eng = FakeEngine(np.zeros((300, 40), np.int64), None)
    h = head(engine=eng).from_features(torch.randn(6, 8), [4, 0, 2, 0, 4, 1])
    for step in [(257, 20), (200, 33)]:
        with pytest.raises(ValueError, match="at most 256 betas and 32 alphas"):
            h.search_hp(torch.randn(12, 8), torch.arange(12) % 5, step=step)
    assert not eng.search_calls


def test_ordered_pass_of_the_device_loader():
    """The cache is built from DeviceLoader.ordered(): every item once in dataset order, the remainder of the last batch included,
    through the train transform, while `for batch in loader` keeps its permutations and drop_last."""
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.data import Datum, DeviceLoader
    from mvlpt_amd.tip_adapter import _Batches
    cfg = get_cfg_default()
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    items = [Datum(impath=f"{i}.jpg", label=i % 3, domain=0, classname=str(i % 3)) for i in range(10)]
    loader = DeviceLoader(cfg, items, train=True)
    with pytest.raises(RuntimeError, match="not bound"):
        loader.ordered()
    draws = []

    class Transform:
        @staticmethod
        def from_resident(image_set, idx):
            draws.append(len(draws))                      # a fresh draw per batch
            return torch.tensor(idx, dtype=torch.float32).view(-1, 1) + 0.01 * draws[-1]

    loader.transform, loader.image_set = Transform, object()
    shuffled = [b["label"].tolist() for b in loader], [b["label"].tolist() for b in loader]
    assert len(shuffled[0]) == 2 and shuffled[0] != shuffled[1]          # drop_last and a new permutation: not what a cache wants
    epoch = loader.epoch
    tr = SimpleNamespace(parse_batch_train=lambda b: (b["img"], b["label"], None))
    wrapped = _Batches(tr, loader, ordered=True)
    passes = [list(wrapped), list(wrapped)]
    assert len(wrapped) == 3 and loader.epoch == epoch
    for p in passes:
        assert [lab.tolist() for _, lab in p] == [[0, 1, 2, 0], [1, 2, 0, 1], [2, 0]]
        assert torch.cat([img for img, _ in p]).round().view(-1).tolist() == list(range(10))
    assert not torch.equal(passes[0][0][0], passes[1][0][0])             # the transform drew again
    assert len(_Batches(tr, loader)) == 2                                # fit keeps the shuffled loader
    batches = [{"img": torch.zeros(2, 1), "label": torch.tensor([1, 0])}]
    assert [lab.tolist() for _, lab in _Batches(tr, batches, ordered=True)] == [[1, 0]]      # a list has no other order


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_registration():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tools_train_for_tip", os.path.join(ROOT, "tools", "train.py"))
    launcher = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(launcher)
    from mvlpt_amd.tip_adapter import TipAdapter
    from mvlpt_amd.trainer import MVLPT
    from mvlpt_amd.zsclip import ZeroshotCLIP
    assert "TipAdapter" in launcher.TRAINERS and "TipAdapter" not in launcher.EVAL_ONLY_TRAINERS      # it has a train()
    assert launcher.trainer_class("TipAdapter") is TipAdapter and TipAdapter.__name__ == "TipAdapter"
    assert issubclass(TipAdapter, ZeroshotCLIP) and TipAdapter.test is MVLPT.test


def _cfg():
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    return cfg


def test_trainer_refusals_name_their_key():
    from mvlpt_amd.tip_adapter import TipAdapter, tip_settings
    tr = object.__new__(TipAdapter)
    TipAdapter.check_cfg(tr, _cfg())
    s = tip_settings(_cfg())
    assert s["augment_epoch"] == 10 and s["search"] and not s["finetune"] and s["step"] == [200, 20]
    for key, value, pattern in [("TRAINER.MVLPT.VPT.N_CTX", 4, r"TRAINER\.MVLPT\.VPT\.N_CTX"), ("DATASET.MULTITASK", True, r"DATASET\.MULTITASK"),
                                ("TRAINER.TIP.AUGMENT_EPOCH", 0, r"TRAINER\.TIP\.AUGMENT_EPOCH"),
                                ("TRAINER.TIP.SEARCH_STEP", [200], r"TRAINER\.TIP\.SEARCH_S"), ("TRAINER.TIP.LR", 0.0, r"TRAINER\.TIP\.LR")]:
        cfg = _cfg()
        node = cfg
        *path, leaf = key.split(".")
        for p in path:
            node = node[p]
        node[leaf] = value
        with pytest.raises(ValueError, match=pattern):
            TipAdapter.check_cfg(tr, cfg)
    cfg = _cfg()
    cfg.TRAINER.TIP.FINETUNE, cfg.TRAINER.TIP.TRAIN_EPOCH = True, 0
    with pytest.raises(ValueError, match=r"TRAINER\.TIP\.TRAIN_EPOCH"):
        TipAdapter.check_cfg(tr, cfg)
    cfg = _cfg()
    cfg.TRAINER.ZSCLIP.TEMPLATES = ["a {}.", "the {}."]           # one text classifier: ZeroshotCLIP's rule
    with pytest.raises(ValueError):
        TipAdapter.check_cfg(tr, cfg)
    with pytest.raises(RuntimeError, match="train"):
        TipAdapter.forward_backward(tr, None)
