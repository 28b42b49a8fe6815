"""Host side of mvlpt_amd.data (no device): readers, few-shot draws, class subsampling, multitask composition, the loaders' order and
length, binding, thread lifetime and the descriptors of the resident route, against a stub engine that records its arguments."""
import json
import os
import random
import threading
import types

import pytest
import torch

from mvlpt_amd.config import get_cfg_default
from mvlpt_amd.data import (Datum, DeviceDataManager, DeviceLoader, few_shot, rank_seed, read_folders, read_split_json,
                            subsample_classes)
from mvlpt_amd.transforms import DeviceTransform
from tests.data_util import CLASSES, COUNTS, write_dataset


class StubEngine:
    """records what the transform hands to the engine; returns zeros of the right shape"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def _record(self, src, descs, size):
        self.calls.append({"src": src, "descs": [(int(d.offset), int(d.height), int(d.width)) for d in descs]})
        return torch.zeros(len(descs), 3, size, size)

    def preprocess(self, src, descs, size, mean, std, out_dtype=torch.float32, want_u8=False):
        return self._record(src, descs, size)

    def preprocess_aug(self, src, descs, augs, size, mean, std, out_dtype=torch.float32, want_u8=False, fill_outside=False):
        return self._record(src, descs, size)


def make_cfg(sources, batch=4, test_batch=4, workers=2):
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.DATASET.SOURCES = sources
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = batch
    cfg.DATALOADER.TEST.BATCH_SIZE = test_batch
    cfg.DATALOADER.NUM_WORKERS = workers
    cfg.DATALOADER.RESIDENT_BYTES = 0          # the streaming route with Pillow decodes needs no device
    cfg.DATALOADER.DECODE = "host"
    return cfg


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("images"))
    return root, write_dataset(root)


def test_readers_agree_and_are_consistent(dataset):
    root, items = dataset
    by_folder = read_folders(root)
    by_split = read_split_json(os.path.join(root, "split.json"), root)
    for got_f, got_s, split in zip(by_folder, by_split, ("train", "val", "test")):
        want = [Datum(p, lab, 0, c) for p, lab, c in items[split]]
        assert got_f == want and got_s == want
        assert len(want) == 3 * COUNTS[split]
    classes = sorted(CLASSES)
    for it in by_folder[0] + by_folder[1] + by_folder[2]:
        assert classes[it.label] == it.classname and os.path.isfile(it.impath) and it.domain == 0


def test_read_folders_without_val(tmp_path):
    root = str(tmp_path)
    write_dataset(root)
    import shutil
    shutil.rmtree(os.path.join(root, "val"))
    train, val, test = read_folders(root)
    assert val == [] and len(train) == 18 and len(test) == 9


def test_few_shot_draws():
    items = [Datum(f"a{k}", 0) for k in range(10)] + [Datum(f"c{k}", 2) for k in range(3)] + [Datum(f"b{k}", 1) for k in range(7)]
    a = few_shot(items, 4, random.Random(5))
    b = few_shot(items, 4, random.Random(5))
    c = few_shot(items, 4, random.Random(6))
    assert a == b and a != c                                            # deterministic in the seed
    assert [it.label for it in a] == [0] * 4 + [1] * 4 + [2] * 3        # ascending labels; the short class is kept whole
    assert len(set(a)) == len(a) and set(a) <= set(items)               # without replacement
    assert [it for it in a if it.label == 2] == [it for it in items if it.label == 2]
    assert few_shot(items, 0, random.Random(1)) == items


def test_subsample_classes_odd_count():
    mk = lambda n: [Datum(f"{n}{k}", k % 5, 0, f"c{k % 5}") for k in range(10)]   # noqa: E731
    train, val, test = mk("t"), mk("v"), mk("s")
    base = subsample_classes(train, val, test, "base")
    new = subsample_classes(train, val, test, "new")
    for part in base:                                                   # ceil(5 / 2) = 3 classes, labels kept
        assert sorted({it.label for it in part}) == [0, 1, 2] and all(it.classname == f"c{it.label}" for it in part)
    for part in new:                                                    # the other 2, relabelled from 0
        assert sorted({it.label for it in part}) == [0, 1] and all(it.classname == f"c{it.label + 3}" for it in part)
    assert [len(p) for p in base] == [6, 6, 6] and [len(p) for p in new] == [4, 4, 4]
    assert subsample_classes(train, val, test, "all") == (train, val, test)
    with pytest.raises(ValueError):
        subsample_classes(train, val, test, "some")


def test_multitask_composition(dataset, tmp_path):
    root, items = dataset
    root2 = str(tmp_path / "second")
    write_dataset(root2, seed=1)
    cfg = make_cfg([["pets", os.path.join(root, "split.json"), root], ["cars", "", root2]])
    cfg.DATASET.SUBSAMPLE_CLASSES = "all"
    dm = DeviceDataManager(cfg)
    classes = sorted(CLASSES)
    assert dm.num_classes == dm._num_classes == 6 and dm.num_classes_list == [3, 3] and dm.classnames == classes + classes
    assert dm._task_names == ["pets", "cars"] and dm._id2task == {0: "pets", 1: "cars"}
    assert dm._task_class_idx == {"pets": (0, 3), "cars": (3, 6)} and dm._labelmap == {"pets": classes, "cars": classes}
    assert sorted(dm.lab2cname) == list(range(6)) and [dm.lab2cname[k] for k in range(6)] == classes + classes
    assert dm.dataset.classnames == dm.classnames and dm.train_loader_u is None and dm.num_source_domains == 1
    for loader, split in ((dm.train_loader_x, "train"), (dm.val_loader, "val"), (dm.test_loader, "test")):
        n = 3 * COUNTS[split]
        assert len(loader.dataset) == 2 * n
        first, second = loader.dataset[:n], loader.dataset[n:]
        assert [(it.impath, it.label, it.domain) for it in first] == [(p, lab, 0) for p, lab, _ in items[split]]
        assert all(it.domain == 1 and 3 <= it.label < 6 and it.impath.startswith(root2) for it in second)
        assert all(dm.lab2cname[it.label] == it.classname for it in loader.dataset)
    # base classes of each source: 2 of 3, relabelled and shifted
    cfg.DATASET.SUBSAMPLE_CLASSES = "base"
    dm = DeviceDataManager(cfg)
    assert dm.num_classes_list == [2, 2] and dm._task_class_idx == {"pets": (0, 2), "cars": (2, 4)}
    assert dm.classnames == classes[:2] * 2 and {it.label for it in dm.test_loader.dataset} == {0, 1, 2, 3}


def test_sources_come_from_the_command_line(dataset):
    root, _ = dataset
    cfg = get_cfg_default()
    assert cfg.DATASET.SOURCES == [] and cfg.DATASET.SUBSAMPLE_CLASSES == "all" and cfg.DATALOADER.DECODE == "device"
    assert cfg.DATALOADER.RESIDENT_BYTES == 16 * 2 ** 30
    cfg.merge_from_list(["DATASET.SOURCES", json.dumps([["pets", "", root]]), "DATALOADER.RESIDENT_BYTES", "0"])
    assert cfg.DATASET.SOURCES == [["pets", "", root]] and cfg.DATALOADER.RESIDENT_BYTES == 0


def test_train_order_length_and_eval_order(dataset):
    root, items = dataset
    cfg = make_cfg([["pets", "", root]], batch=4, test_batch=4)
    dm = DeviceDataManager(cfg)
    tl = dm.train_loader_x
    assert len(tl) == 18 // 4 and tl.batch_size == 4 and len(dm.test_loader) == 3 and len(dm.val_loader) == 2      # drop_last / partial
    assert tl.order(0) != tl.order(1) and sorted(tl.order(0)) == list(range(18))
    assert tl.order(3) == torch.randperm(18, generator=torch.Generator().manual_seed(cfg.SEED + 3)).tolist()
    assert tl.order(0) != DeviceLoader(cfg, tl.dataset, train=True, rank=1).order(0) and rank_seed(7, 0) == 7
    dm.bind(StubEngine())
    dm2 = DeviceDataManager(cfg)
    dm2.bind(StubEngine())
    epochs = [[b["impath"] for b in tl] for _ in range(2)]
    again = [[b["impath"] for b in dm2.train_loader_x] for _ in range(2)]
    assert epochs == again and epochs[0] != epochs[1]                   # equal seeds, equal order; a fresh one per epoch
    paths = [p for p, _, _ in items["train"]]
    for e, ep in enumerate(epochs):
        assert [len(b) for b in ep] == [4] * 4
        assert [p for b in ep for p in b] == [paths[i] for i in tl.order(e)[:16]]
    # evaluation: every item once, in order, the last batch partial
    got = list(dm.test_loader)
    assert [len(b["impath"]) for b in got] == [4, 4, 1]
    assert [p for b in got for p in b["impath"]] == [p for p, _, _ in items["test"]]
    assert torch.cat([b["label"] for b in got]).tolist() == [lab for _, lab, _ in items["test"]]
    assert got[0]["img"].shape == (4, 3, 32, 32) and got[0]["label"].dtype == torch.int64 and got[0]["domain"].tolist() == [0] * 4
    assert [p for b in dm.test_loader for p in b["impath"]] == [p for p, _, _ in items["test"]]      # and again the same


def test_unbound_loader_raises(dataset):
    root, _ = dataset
    dm = DeviceDataManager(make_cfg([["pets", "", root]]))
    for loader in (dm.train_loader_x, dm.val_loader, dm.test_loader):
        with pytest.raises(RuntimeError, match="not bound"):
            iter(loader)
        with pytest.raises(RuntimeError, match="not bound"):
            for _ in loader:
                pass


def test_no_sources_and_no_manager_is_still_an_error(tmp_path):
    from mvlpt_amd.trainer import MVLPT
    cfg = make_cfg([])
    cfg.OUTPUT_DIR = str(tmp_path)
    with pytest.raises(ValueError, match="pass a data manager"):
        MVLPT(cfg)


def test_reader_threads_end_with_the_iteration(dataset):
    root, _ = dataset
    from mvlpt_amd.trainer import LookAheadLoader
    dm = DeviceDataManager(make_cfg([["pets", "", root]], batch=2, workers=3))
    dm.bind(StubEngine())
    start = threading.active_count()
    owner = types.SimpleNamespace(next_batch=None)
    for loader in (dm.train_loader_x, LookAheadLoader(dm.train_loader_x, owner)):
        assert len(list(loader)) == 9                                   # a full iteration
        assert threading.active_count() == start
        seen_threads = 0
        for k, _ in enumerate(loader):                                  # an early break
            seen_threads = max(seen_threads, threading.active_count() - start)
            if k == 1:
                break
        assert seen_threads >= 1 and threading.active_count() == start
        with pytest.raises(KeyError):                                   # an exception in the consumer
            for k, _ in enumerate(loader):
                if k == 2:
                    raise KeyError("consumer")
        assert threading.active_count() == start
    it = iter(dm.train_loader_x)                                        # an iterator somebody keeps: close() joins its threads
    next(it)
    assert threading.active_count() > start
    dm.train_loader_x.close()
    assert threading.active_count() == start


@pytest.mark.parametrize("transforms", [["random_resized_crop", "random_flip", "normalize"],
                                        ["random_crop", "random_flip", "colorjitter", "cutout", "normalize"]])
def test_from_resident_descriptors(transforms):
    shapes = [(17, 23), (64, 48), (23, 17), (40, 40), (31, 64)]
    offsets, total = [], 2 ** 32 + 5                                    # a set that begins beyond 32 bits
    for h, w in shapes:
        offsets.append(total)
        total += h * w * 3
    image_set = types.SimpleNamespace(buf=torch.empty(0, dtype=torch.uint8), offsets=offsets, shapes=shapes)
    order = [3, 0, 4, 4, 1, 2]
    eng = StubEngine()
    tr = DeviceTransform(eng, size=32, train=True, transforms=transforms, generator=torch.Generator().manual_seed(11))
    out = tr.from_resident(image_set, order)
    assert out.shape == (6, 3, 32, 32) and len(eng.calls) == 1 and eng.calls[0]["src"] is image_set.buf
    assert eng.calls[0]["descs"] == [(offsets[i], *shapes[i]) for i in order]
    # the draws are those of __call__ / describe_aug for images of these sizes
    ref = DeviceTransform(eng, size=32, train=True, transforms=transforms, generator=torch.Generator().manual_seed(11))
    want, want_aug, _ = ref.describe_aug([shapes[i] for i in order])
    tr2 = DeviceTransform(eng, size=32, train=True, transforms=transforms, generator=torch.Generator().manual_seed(11))
    seen = {}
    eng.preprocess = eng.preprocess_aug = lambda src, descs, *a, **k: seen.setdefault("d", (descs, a[0] if tr2.augments else None)) and torch.zeros(1)
    tr2.from_resident(image_set, order)
    fields = ("crop_top", "crop_left", "crop_height", "crop_width", "resize_height", "resize_width", "out_top", "out_left", "flip")
    for d, w in zip(seen["d"][0], want):
        assert [getattr(d, f) for f in fields] == [getattr(w, f) for f in fields]
    if want_aug is not None:
        assert bytes(seen["d"][1]) == bytes(want_aug)
