"""mvlpt_amd.data on the device: every route of the loaders (resident, streaming, host decode) gives, bit for bit, the batches
`DeviceTransform.__call__` gives for the Pillow-decoded files in the same order with the same generator seed; the resident set's
accounting and its end; an image beyond 2^32 bytes of a resident buffer; and the trainers fed from `DATASET.SOURCES` against the same
trainers fed the same batches from plain lists.  The loader adds no arithmetic, so every comparison is an equality."""
import os
import types

import pytest
import torch

from tests.data_util import N_HOST_TRAIN, pillow_arrays, write_dataset

pytestmark = pytest.mark.gpu

DEFAULT = ["random_resized_crop", "random_flip", "normalize"]
AUGMENTED = ["random_crop", "random_flip", "colorjitter", "cutout", "normalize"]
B_TRAIN, B_TEST, EPOCHS = 4, 4, 2


@pytest.fixture(scope="module")
def eng():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    return Engine(ARCHS["tiny"], "fp16")


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("images"))
    return root, write_dataset(root)


def make_cfg(sources, transforms=DEFAULT, resident=16 * 2 ** 30, decode="device"):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.MODEL.BACKBONE.NAME = "tiny"
    cfg.INPUT.SIZE = (32, 32)
    cfg.INPUT.TRANSFORMS = list(transforms)
    cfg.DATASET.SOURCES = sources
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = B_TRAIN
    cfg.DATALOADER.TEST.BATCH_SIZE = B_TEST
    cfg.DATALOADER.NUM_WORKERS = 2
    cfg.DATALOADER.RESIDENT_BYTES = resident
    cfg.DATALOADER.DECODE = decode
    return cfg


def reference_batches(eng, cfg, items, train, epochs=1):
    """[epoch][batch] of `DeviceTransform.__call__` on the Pillow-decoded files of `items` ((path, label, domain) triples): the order of
    torch.Generator().manual_seed(SEED + epoch) and drop_last for training, sequential with a partial last batch otherwise; ONE
    generator seeded SEED draws the transform parameters, batch after batch."""
    from mvlpt_amd.transforms import build_device_transform
    arrays = pillow_arrays([p for p, _, _ in items])
    labels = torch.tensor([lab for _, lab, _ in items], dtype=torch.int64)
    domains = torch.tensor([d for _, _, d in items], dtype=torch.int64)
    tr = build_device_transform(cfg, eng, train=train, generator=torch.Generator().manual_seed(cfg.SEED) if train else None)
    n, B = len(items), B_TRAIN if train else B_TEST
    out = []
    for e in range(epochs):
        order = torch.randperm(n, generator=torch.Generator().manual_seed(cfg.SEED + e)).tolist() if train else list(range(n))
        nb = n // B if train else (n + B - 1) // B
        ep = []
        for k in range(nb):
            idx = order[k * B:(k + 1) * B]
            ep.append({"img": tr([arrays[i] for i in idx]), "label": labels[idx].cuda(), "domain": domains[idx],
                       "impath": [items[i][0] for i in idx]})
        out.append(ep)
    return out


def triples(rows, domain=0):
    return [(p, lab, domain) for p, lab, _ in rows]


_REF = {}


def reference(eng, dataset, transforms):
    """the reference batches of the one-source dataset, computed once per transform list and shared"""
    root, items = dataset
    key = tuple(transforms)
    if key not in _REF:
        cfg = make_cfg([["pets", "", root]], transforms)
        _REF[key] = {"train": reference_batches(eng, cfg, triples(items["train"]), True, EPOCHS),
                     "val": reference_batches(eng, cfg, triples(items["val"]), False)[0],
                     "test": reference_batches(eng, cfg, triples(items["test"]), False)[0]}
    return _REF[key]


def assert_batches_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["impath"] == w["impath"]
        assert g["img"].is_cuda and g["label"].is_cuda and g["label"].dtype == torch.int64 and g["domain"].dtype == torch.int64
        assert torch.equal(g["label"], w["label"]) and torch.equal(g["domain"], w["domain"])
        assert g["img"].shape == w["img"].shape and torch.equal(g["img"], w["img"])


def bound_manager(eng, cfg):
    from mvlpt_amd.data import DeviceDataManager
    dm = DeviceDataManager(cfg)
    dm.bind(eng)
    return dm


# ------------------------------------------------------------------------------------------------ 1-3, 6: the routes
@pytest.mark.parametrize("transforms", [DEFAULT, AUGMENTED], ids=["default", "augmented"])
@pytest.mark.parametrize("route", ["resident", "streaming", "host_decode", "host_decode_streaming"])
def test_every_route_gives_the_reference_batches(eng, dataset, transforms, route):
    root, _ = dataset
    ref = reference(eng, dataset, transforms)
    cfg = make_cfg([["pets", "", root]], transforms, resident=0 if "streaming" in route else 16 * 2 ** 30,
                   decode="host" if "host" in route else "device")
    dm = bound_manager(eng, cfg)
    resident = "streaming" not in route
    assert all((s is not None) == resident for s in dm.image_sets.values()) and set(dm.image_sets) == {"train", "val", "test"}
    for e in range(EPOCHS):
        assert_batches_equal(list(dm.train_loader_x), ref["train"][e])
    assert_batches_equal(list(dm.test_loader), ref["test"])            # sequential, the last batch partial, centre crop
    assert_batches_equal(list(dm.val_loader), ref["val"])
    assert [len(b["impath"]) for b in ref["test"]] == [4, 4, 1] and len(dm.test_loader) == 3 and len(dm.train_loader_x) == 4


def test_budget_is_spent_in_order_train_val_test(eng, dataset):
    root, items = dataset
    need = {s: sum(a.size for a in pillow_arrays([p for p, _, _ in items[s]])) for s in items}
    dm = bound_manager(eng, make_cfg([["pets", "", root]], resident=need["train"] + need["val"] + need["test"] - 1))
    assert dm.image_sets["train"] is not None and dm.image_sets["val"] is not None and dm.image_sets["test"] is None
    assert dm.resident_bytes == need["train"] + need["val"]
    assert_batches_equal(list(dm.test_loader), reference(eng, dataset, DEFAULT)["test"])


# ------------------------------------------------------------------------------------------------ 4: accounting
def test_resident_set_accounting_and_its_last_image(eng, dataset):
    root, items = dataset
    dm = bound_manager(eng, make_cfg([["pets", "", root]]))
    for split in ("train", "val", "test"):
        s = dm.image_sets[split]
        arrays = pillow_arrays([p for p, _, _ in items[split]])
        assert s.resident_bytes == sum(a.size for a in arrays) == s.buf.numel()
        assert s.shapes == [a.shape[:2] for a in arrays]
        assert s.n_host == (N_HOST_TRAIN if split == "train" else 0) and s.n_corrupt == 0 and s.n_device == len(arrays) - s.n_host
        last = s.buf[s.offsets[-1]:].cpu()
        assert last.numel() == arrays[-1].size and torch.equal(last, torch.from_numpy(arrays[-1].copy()).reshape(-1))
        assert torch.equal(s.buf.cpu(), torch.cat([torch.from_numpy(a.copy()).reshape(-1) for a in arrays]))


# ------------------------------------------------------------------------------------------------ 5: beyond 2^32
def test_an_image_beyond_4_gib_of_a_resident_buffer(eng, dataset):
    from mvlpt_amd import jpeg
    from mvlpt_amd.transforms import DeviceTransform
    _, items = dataset
    paths = [p for p, _, _ in items["train"] if p.endswith(".jpg")]
    blobs = [open(p, "rb").read() for p in paths]
    infos = [jpeg.probe(b) for b in blobs]
    pick = [next(k for k, f in enumerate(infos) if (f.height, f.width) == hw and f.route == 0) for hw in ((17, 23), (23, 17))]
    blobs, infos = [blobs[k] for k in pick], [infos[k] for k in pick]
    assert infos[1].h_samp == 2 and infos[1].v_samp == 2               # the 4:2:0 file with odd sizes
    shapes = [(f.height, f.width) for f in infos]
    low, low_offsets, _, status = jpeg.decode_batch(eng, blobs, infos=infos)
    assert not status.cpu().any()
    total = 2 ** 32 + 2 ** 16
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")          # uninitialised: only the two images are ever read
    first = 2 ** 32 + 7
    offsets = [first, first + shapes[0][0] * shapes[0][1] * 3]
    assert offsets[1] + shapes[1][0] * shapes[1][1] * 3 <= total
    _, st = jpeg.decode_into(eng, blobs, buf, offsets, shapes, infos)
    assert not st.any()
    for off, lo, (h, w) in zip(offsets, low_offsets, shapes):
        assert torch.equal(buf[off:off + h * w * 3], low[lo:lo + h * w * 3])
    order = [1, 0, 0, 1]
    for transforms in (DEFAULT, AUGMENTED):
        far = DeviceTransform(eng, size=32, transforms=transforms, generator=torch.Generator().manual_seed(4)).from_resident(
            types.SimpleNamespace(buf=buf, offsets=offsets, shapes=shapes), order)
        near = DeviceTransform(eng, size=32, transforms=transforms, generator=torch.Generator().manual_seed(4)).from_resident(
            types.SimpleNamespace(buf=low, offsets=low_offsets, shapes=shapes), order)
        assert torch.equal(far, near)
    del buf


# ------------------------------------------------------------------------------------------------ 7, 8: the trainers
class EpochLists:
    """a train loader over precomputed batches: epoch e of the lists at the e-th iteration"""

    def __init__(self, epochs):
        self.epochs, self.at = epochs, 0

    def __len__(self):
        return len(self.epochs[0])

    def __iter__(self):
        ep = self.epochs[self.at]
        self.at += 1
        return iter(ep)


class ListDataManager:
    """plain lists of batches behind the attribute surface of `like` (a DeviceDataManager)"""

    def __init__(self, like, train_epochs, val, test):
        for name in ("num_classes", "_num_classes", "classnames", "lab2cname", "num_source_domains", "num_classes_list", "_task_names",
                     "_id2task", "_task_class_idx", "_labelmap"):
            setattr(self, name, getattr(like, name))
        self.dataset = self
        self.train_loader_x, self.train_loader_u, self.val_loader, self.test_loader = EpochLists(train_epochs), None, val, test


def run_trainer(make, epochs):
    """(per-step losses, test result, per-task results, trainer) of a fresh trainer"""
    torch.manual_seed(0)                                               # the same prompt initialisation in every run
    tr = make()
    losses = []
    if epochs:
        step = tr.forward_backward
        tr.forward_backward = lambda batch: (lambda s: (losses.append(s["loss"]), s)[1])(step(batch))
    for tr.epoch in range(epochs):
        tr.run_epoch()
    acc = tr.test()
    return [float(v) for v in losses], acc, dict(tr.last_task_results), tr


def trainer_cfg(cfg, tmp_path, name):
    cfg.TRAINER.NAME = name
    cfg.OUTPUT_DIR = str(tmp_path)
    cfg.OPTIM.MAX_EPOCH, cfg.OPTIM.LR, cfg.OPTIM.WARMUP_EPOCH = EPOCHS, 0.05, 0
    cfg.TRAIN.PRINT_FREQ = 10 ** 9
    cfg.TRAINER.MVLPT.COOP.N_CTX, cfg.TRAINER.MVLPT.PROJECT_DIM = 4, 64
    cfg.TRAINER.MVLPT.STEP_PIPELINING = True
    cfg.TRAINER.COCOOP.N_CTX = 4
    return cfg


@pytest.mark.parametrize("name", ["MVLPT", "CoCoOp", "ZeroshotCLIP"])
def test_trainers_from_sources_equal_the_list_fed_run(eng, dataset, tmp_path, name):
    from mvlpt_amd.cocoop import CoCoOp
    from mvlpt_amd.data import DeviceDataManager
    from mvlpt_amd.trainer import MVLPT, LookAheadLoader
    from mvlpt_amd.weights import ARCHS, make_state_dict
    from mvlpt_amd.zsclip import ZeroshotCLIP
    root, _ = dataset
    cls = {"MVLPT": MVLPT, "CoCoOp": CoCoOp, "ZeroshotCLIP": ZeroshotCLIP}[name]
    sd = make_state_dict(ARCHS["tiny"], seed=9, include_token_embedding=name == "ZeroshotCLIP")
    epochs = 0 if name == "ZeroshotCLIP" else EPOCHS
    cfg = trainer_cfg(make_cfg([["pets", "", root]]), tmp_path, name)
    got = run_trainer(lambda: cls(cfg, clip_state_dict=sd), epochs)     # no data manager: DATASET.SOURCES alone
    tr = got[3]
    assert isinstance(tr.dm, DeviceDataManager) and tr.dm.image_sets["train"] is not None
    if name == "MVLPT":
        assert isinstance(tr.train_loader_x, LookAheadLoader) and tr.train_loader_x.hits == EPOCHS * 3
    ref = reference(eng, dataset, DEFAULT)
    cfg2 = trainer_cfg(make_cfg([]), tmp_path, name)
    want = run_trainer(lambda: cls(cfg2, dm=ListDataManager(tr.dm, ref["train"], ref["val"], ref["test"]), clip_state_dict=sd), epochs)
    assert len(got[0]) == epochs * 4 and got[0] == want[0], (got[0], want[0])
    assert got[1] == want[1] and 0.0 <= got[1] <= 100.0


def test_multitask_trainer_from_two_sources(eng, dataset, tmp_path):
    from mvlpt_amd.trainer import MVLPT
    from mvlpt_amd.weights import ARCHS, make_state_dict
    root, items = dataset
    root2 = str(tmp_path / "second")
    items2 = write_dataset(root2, seed=1)
    sd = make_state_dict(ARCHS["tiny"], seed=9)

    def cfg_of(sources):
        cfg = trainer_cfg(make_cfg(sources), tmp_path, "MVLPT")
        cfg.DATASET.MULTITASK = cfg.DATASET.MULTITASK_LABEL_PERTASK = True
        return cfg
    cfg = cfg_of([["pets", os.path.join(root, "split.json"), root], ["cars", "", root2]])
    got = run_trainer(lambda: MVLPT(cfg, clip_state_dict=sd), 1)
    both = {s: triples(items[s]) + [(p, lab + 3, 1) for p, lab, _ in items2[s]] for s in ("train", "val", "test")}
    ref = {"train": reference_batches(eng, cfg, both["train"], True, 1), "val": reference_batches(eng, cfg, both["val"], False)[0],
           "test": reference_batches(eng, cfg, both["test"], False)[0]}
    cfg2 = cfg_of([])
    want = run_trainer(lambda: MVLPT(cfg2, dm=ListDataManager(got[3].dm, ref["train"], ref["val"], ref["test"]), clip_state_dict=sd), 1)
    assert len(got[0]) == 36 // B_TRAIN and got[0] == want[0], (got[0], want[0])
    assert set(got[2]) == {"pets", "cars"} and got[2] == want[2] and got[1] == want[1]
