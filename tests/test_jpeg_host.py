"""Host side of the device JPEG decode, no GPU: `mvlpt_jpeg_probe` (the parser of csrc/jpeg_core.h through the C ABI) against Pillow
and against tests/jpeg_ref.py over the whole fixture, the route of every fallback case, the workspace arithmetic, and
`DeviceTransform.describe_encoded` / `from_encoded` drawing what `__call__` draws."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))


@pytest.fixture(scope="module")
def jpeg():
    if not os.path.isfile(os.path.join(ROOT, "mvlpt_amd", "libmvlpt_hip.so")):
        import __graft_entry__ as g
        g.build()
    from mvlpt_amd import jpeg
    return jpeg


def test_probe_equals_pillow_and_ref(golden, jpeg):
    modes = {1: "L", 3: "RGB", 4: "CMYK"}
    for k, name in enumerate(golden["names"]):
        blob = golden[f"jpeg_{k}"].tobytes()
        f, P = jpeg.probe(blob), jpeg_ref.parse(blob)
        im = Image.open(io.BytesIO(blob))                          # reads the headers only: the cut file opens too
        assert (f.width, f.height) == im.size and modes[f.components] == im.mode and f.components == im.layers, name
        assert (f.h_samp, f.v_samp) == tuple(im.layer[0][1:3]), name
        assert f.route == P.route and f.restart_interval == P.restart_interval, name
        assert f.n_segments == (P.n_segments if P.route == 0 else 0), name
        assert (f.route != 0) == (golden["kinds"][k] == 1), name


def test_fallback_reasons(golden, jpeg):
    names = list(golden["names"])
    for name, reason in (("fallback_progressive", "frame"), ("fallback_cmyk", "colour"), ("fallback_440", "sampling")):
        assert jpeg.probe(golden[f"jpeg_{names.index(name)}"].tobytes()).reason == reason


def test_probe_of_damaged_headers(jpeg):
    buf = io.BytesIO()
    Image.fromarray(np.zeros((9, 11, 3), np.uint8)).save(buf, "JPEG", subsampling=0, restart_marker_blocks=1)
    blob = buf.getvalue()
    assert jpeg.probe(blob).reason == "device" and jpeg.probe(blob).n_segments == 4
    assert jpeg.probe(b"").reason == "malformed" and jpeg.probe(blob[:1]).reason == "malformed" and jpeg.probe(b"\x89PNG" + blob).reason == "malformed"
    k = blob.index(b"\xff\xdb")
    assert jpeg.probe(blob[:k + 2] + b"\xff\xff" + blob[k + 4:]).reason == "malformed"           # a marker length that runs past the file
    for cut in range(2, blob.index(b"\xff\xda") + 8):                                            # every cut inside the headers
        assert jpeg.probe(blob[:cut]).reason == "malformed"
    k = blob.index(b"\xff\xd1")
    assert jpeg.probe(blob[:k + 1] + b"\xd2" + blob[k + 2:]).reason == "restart"                 # RST1 -> RST2: out of sequence
    assert jpeg.probe(blob[:k] + blob[k + 2:]).reason == "restart"                               # one marker fewer
    k = blob.index(b"\xff\xc4")
    assert jpeg.probe(blob[:k] + blob[k + 2 + blob[k + 2] * 256 + blob[k + 3]:]).reason == "tables"   # the first DHT removed


def test_workspace_bytes(golden, jpeg):
    names = list(golden["names"])
    f = jpeg.probe(golden[f"jpeg_{names.index('100x75_smooth_420_q90')}"].tobytes())
    g = jpeg.probe(golden[f"jpeg_{names.index('fallback_cmyk')}"].tobytes())
    blocks = 7 * 5 * 6                                             # 100 x 75 at 4:2:0: 7 x 5 MCUs of 4 + 1 + 1 blocks
    one = jpeg.workspace_bytes([f])
    assert blocks * (128 + 64) <= one <= blocks * (128 + 64) + 8 * 256 + 4096
    assert jpeg.workspace_bytes([f, g]) == one and jpeg.workspace_bytes([g]) == 0 and jpeg.workspace_bytes([]) == 0
    assert jpeg.workspace_bytes([f, f]) > one


@pytest.mark.parametrize("kwargs", [dict(train=True), dict(train=False), dict(train=False, center_crop=False),
                                    dict(train=True, transforms=("random_crop", "random_flip", "colorjitter", "randomgrayscale", "cutout",
                                                                 "normalize"))])
def test_from_encoded_draws_what_call_draws(golden, jpeg, kwargs):
    from mvlpt_amd.transforms import DeviceTransform
    names = list(golden["names"])
    picks = [names.index(n) for n in ("37x45_noise_420_q90", "100x75_smooth_gray_q90", "fallback_progressive", "9x50_noise_422_q75rst1",
                                      "fallback_cmyk", "33x16_smooth_444_q30opt")]
    blobs = [golden[f"jpeg_{k}"].tobytes() for k in picks]
    arrays = [np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in blobs]
    a = DeviceTransform(None, size=32, generator=torch.Generator().manual_seed(7), **kwargs)
    b = DeviceTransform(None, size=32, generator=torch.Generator().manual_seed(7), **kwargs)
    infos, shapes, descs, augs = a.describe_encoded(blobs)
    want_descs, want_augs, _ = b.describe_aug([x.shape[:2] for x in arrays])
    assert shapes == [x.shape[:2] for x in arrays]
    assert bytes(descs) == bytes(want_descs) and (augs is None) == (want_augs is None)
    assert augs is None or bytes(augs) == bytes(want_augs)
    assert torch.equal(a.generator.get_state(), b.generator.get_state())
