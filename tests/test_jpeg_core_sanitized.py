"""The bounds of the JPEG decode are proven on the CPU: tools/jpeg_core_check.cpp runs mvlpt_amd/csrc/jpeg_core.h -- the parser and the
__host__ __device__ functions the kernels of jpeg.hip call -- as a stand-alone program under the address and undefined-behaviour
sanitizers, over every fixture file and a few thousand seeded mutations and truncations of them, in buffers of exactly the sizes the
C ABI computes.  A sanitizer report aborts the program (-fno-sanitize-recover), so exit status 0 is "nothing outside the buffers"."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTATIONS_PER_FILE = 20          # x 196 supported files = 3 920 mutated files with Pillow's verdict, and as many made by the program


def pillow_pixels(blob):
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")).tobytes()
    except Exception:
        return b""


def mutations(blob, rng, count):
    """seeded damage at marker and entropy positions: a header byte replaced, an entropy byte replaced, an entropy bit flipped, a cut
    anywhere, a cut inside the scan"""
    scan = jpeg_ref.parse(blob).segs[0][0]
    n = len(blob)
    for _ in range(count):
        m = bytearray(blob)
        how = int(rng.integers(0, 8))
        if how < 2:
            m[int(rng.integers(0, scan))] = int(rng.integers(0, 256))
        elif how < 4:
            m[int(rng.integers(scan, n))] = int(rng.integers(0, 256))
        elif how < 6:
            m[int(rng.integers(scan, n))] ^= 1 << int(rng.integers(0, 8))
        elif how == 6:
            del m[int(rng.integers(0, n)):]
        else:
            del m[int(rng.integers(scan, n)):]
        yield bytes(m)


def write_cases(path):
    """-> (supported files, mutated files written)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))
    kinds = z["kinds"]
    rng = np.random.default_rng(2024)
    records = []
    for k, kind in enumerate(kinds):
        jpg = z[f"jpeg_{k}"].tobytes()
        records.append((int(kind), jpg, z[f"rgb_{k}"].tobytes() if kind == 0 else b""))
        if kind == 0:
            records += [(3, m, pillow_pixels(m)) for m in mutations(jpg, rng, MUTATIONS_PER_FILE)]
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for kind, jpg, px in records:
            f.write(struct.pack("<III", kind, len(jpg), len(px)) + jpg + px)
    return int((kinds == 0).sum()), sum(r[0] == 3 for r in records)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("jpeg_core") / "jpeg_core_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           os.path.join(ROOT, "mvlpt_amd", "csrc"), os.path.join(ROOT, "tools", "jpeg_core_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler lacks the sanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_fixture_and_mutations_stay_in_bounds(program, tmp_path):
    """Every fixture file decodes to its recorded pixels; every one of the seeded mutations ends with a fallback route, a set status, or
    the pixels Pillow decodes from the same damaged file; the program's own further mutations only have to stay inside the buffers.
    Counted apart and not held to Pillow: damaged values that leave the IDCT's number range (dequantised coefficients or first-pass
    outputs beyond 16 bits, second-pass outputs outside [-512, 511]), where libjpeg's C and SIMD IDCTs differ from each other.  With
    Pillow 12.2.0: 3 920 mutations = 1 776 equal to Pillow, 1 019 flagged, 944 fallback, 110 Pillow cannot read, 71 beyond the range."""
    cases = str(tmp_path / "cases.bin")
    supported, mutated = write_cases(cases)
    assert mutated == supported * MUTATIONS_PER_FILE >= 3000
    r = subprocess.run([program, cases, str(MUTATIONS_PER_FILE), "12345"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    words = r.stdout.split()
    assert words[words.index("failures") + 1] == "0"
    assert int(words[words.index("given-mutations") + 1].rstrip(":")) == mutated
    print(r.stdout.strip())
