"""The views of test-time prompt tuning on the device (-m gpu): mvlpt_amd.transforms.ViewTransform gives, bit for bit, the
concatenation of a train=False transform's output and a train=True transform's `from_resident(set, [i] * (V - 1))` under the same
generator state, in one preprocess launch; the streaming routes (one device decode per file, or one packed upload of decoded arrays)
equal the resident one; and the loaders serve views only where they were asked to."""
import pytest
import torch

from tests.data_util import pillow_arrays, write_dataset

pytestmark = pytest.mark.gpu

V, SIZE, SEED = 5, 32, 11
DEFAULT = ["random_resized_crop", "random_flip", "normalize"]
AUGMENTED = ["random_crop", "random_flip", "colorjitter", "cutout", "normalize"]


@pytest.fixture(scope="module")
def eng():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    return Engine(ARCHS["tiny"], "fp16")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("views"))
    items = write_dataset(root)
    return root, [p for p, _, _ in items["test"]]          # plain 4:4:4 JPEGs: the device decodes them


@pytest.fixture(scope="module")
def resident(eng, files):
    from mvlpt_amd.data import ResidentImageSet, probe_files
    _, paths = files
    return ResidentImageSet(eng, paths, probe_files(paths), "device", 0)


def pair(eng, transforms, seed=SEED):
    from mvlpt_amd.transforms import DeviceTransform
    return (DeviceTransform(eng, size=SIZE, train=False),
            DeviceTransform(eng, size=SIZE, train=True, transforms=transforms, generator=torch.Generator().manual_seed(seed)))


@pytest.mark.parametrize("transforms", [DEFAULT, AUGMENTED], ids=["default", "augmented"])
def test_views_equal_the_test_view_and_the_train_views(eng, resident, transforms):
    from mvlpt_amd.transforms import ViewTransform
    idx = [4, 0, 7]
    got = ViewTransform(*pair(eng, transforms), V).from_resident(resident, idx)
    assert got.shape == (len(idx), V, 3, SIZE, SIZE) and got.is_cuda
    test_t, train_t = pair(eng, transforms)                 # the same generator state, driven by hand, image after image
    for g, i in enumerate(idx):
        want = torch.cat([test_t.from_resident(resident, [i]), train_t.from_resident(resident, [i] * (V - 1))])
        assert torch.equal(got[g], want), (g, i)
    assert not torch.equal(got[0, 1], got[0, 2])            # the train views differ


def test_streaming_routes_equal_the_resident_one(eng, resident, files):
    from mvlpt_amd.transforms import ViewTransform
    _, paths = files
    idx = [2, 8, 5, 0]
    want = ViewTransform(*pair(eng, DEFAULT), V).from_resident(resident, idx)
    blobs = [open(paths[i], "rb").read() for i in idx]
    assert torch.equal(ViewTransform(*pair(eng, DEFAULT), V).from_encoded(blobs), want)              # one decode of the batch
    assert torch.equal(ViewTransform(*pair(eng, DEFAULT), V)(pillow_arrays([paths[i] for i in idx])), want)   # one packed upload


def test_loaders_serve_views_on_request_and_nothing_else_changes(eng, files):
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.data import DeviceDataManager

    def cfg_of(resident_bytes):
        cfg = get_cfg_default()
        cfg.MODEL.BACKBONE.NAME = "tiny"
        cfg.INPUT.SIZE = (SIZE, SIZE)
        cfg.DATASET.SOURCES = [["pets", "", files[0]]]
        cfg.DATALOADER.TRAIN_X.BATCH_SIZE, cfg.DATALOADER.TEST.BATCH_SIZE, cfg.DATALOADER.NUM_WORKERS = 4, 4, 2
        cfg.DATALOADER.RESIDENT_BYTES = resident_bytes
        return cfg
    plain = DeviceDataManager(cfg_of(16 * 2 ** 30))
    plain.bind(eng)
    base_train, base_test = list(plain.train_loader_x), list(plain.test_loader)
    out = {}
    for name, budget in (("resident", 16 * 2 ** 30), ("streaming", 0)):
        dm = DeviceDataManager(cfg_of(budget))
        dm.request_views(V)
        dm.bind(eng)
        assert (dm.image_sets["test"] is not None) == (name == "resident")
        for a, b in zip(list(dm.train_loader_x), base_train):                   # the train batches keep their bits
            assert torch.equal(a["img"], b["img"]) and torch.equal(a["label"], b["label"])
        out[name] = list(dm.test_loader)
        assert [tuple(b["img"].shape) for b in out[name]] == [(4, V, 3, SIZE, SIZE), (4, V, 3, SIZE, SIZE), (1, V, 3, SIZE, SIZE)]
        for a, b in zip(out[name], base_test):                                  # view 0 is the plain test batch
            assert torch.equal(a["img"][:, 0], b["img"]) and torch.equal(a["label"], b["label"]) and a["impath"] == b["impath"]
    for a, b in zip(out["resident"], out["streaming"]):
        assert torch.equal(a["img"], b["img"])
