"""tests/jpeg_ref.py, the numpy restatement of the device's JPEG decode, `==` Pillow: over the whole fixture, and over files encoded on
the spot (so the restatement is held against the Pillow that is installed, not only the one that wrote the fixture)."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))


def test_fixture_has_the_cases(golden):
    names, kinds = list(golden["names"]), golden["kinds"]
    assert (kinds == 0).sum() >= 168 + 8 and (kinds == 1).sum() == 3 and (kinds == 2).sum() == 2
    for s in ("444", "422", "420", "gray"):
        for e in ("q90", "q30opt", "q75rst1", "q100", "q75rstrow"):
            assert any(f"_{s}_{e}" in n for n in names), (s, e)
    assert any(n.startswith("100x75") for n in names)


def test_ref_equals_pillow_on_the_fixture(golden):
    kinds = golden["kinds"]
    for k in np.flatnonzero(kinds == 0):
        rgb, status = jpeg_ref.decode(golden[f"jpeg_{k}"].tobytes())
        assert status == 0 and np.array_equal(rgb, golden[f"rgb_{k}"]), golden["names"][k]


def test_fallback_and_malformed_cases(golden):
    names = list(golden["names"])
    want = {"fallback_progressive": jpeg_ref.ROUTE_FRAME, "fallback_cmyk": jpeg_ref.ROUTE_COLOUR, "fallback_440": jpeg_ref.ROUTE_SAMPLING}
    for name, route in want.items():
        assert jpeg_ref.parse(golden[f"jpeg_{names.index(name)}"].tobytes()).route == route, name
    for name in ("malformed_cut", "malformed_byte"):
        blob = golden[f"jpeg_{names.index(name)}"].tobytes()
        assert jpeg_ref.parse(blob).route == jpeg_ref.ROUTE_DEVICE and jpeg_ref.decode(blob)[1] > 0, name


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (3, 5), (4, 17), (5, 3), (16, 16), (23, 9)])
def test_ref_equals_pillow_on_fresh_files(size):
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    a = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    for sampling in (0, 1, 2, None):
        for kw in (dict(quality=85), dict(quality=50, optimize=True), dict(quality=95, restart_marker_blocks=2)):
            buf = io.BytesIO()
            im = Image.fromarray(a)
            if sampling is None:
                im.convert("L").save(buf, "JPEG", **kw)
            else:
                im.save(buf, "JPEG", subsampling=sampling, **kw)
            rgb, status = jpeg_ref.decode(buf.getvalue())
            assert status == 0
            assert np.array_equal(rgb, np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))), (size, sampling, kw)
