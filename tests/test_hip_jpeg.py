"""Baseline JPEG decode on the device (csrc/jpeg.hip) through the C ABI, -m gpu.  Bar: BIT-EXACT.  The whole decode `==` Pillow's pixels
(tests/golden/jpeg.npz); each stage on its own `==` tests/jpeg_ref.py, the numpy restatement that tests/test_jpeg_ref.py holds to
Pillow.  The bounds of what runs here were proven on the CPU first (tests/test_jpeg_core_sanitized.py), the two malformed files
included."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from tests import jpeg_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    return Engine(ARCHS["tiny"], "fp16")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))
    names = list(z["names"])
    return dict(names=names, kinds=z["kinds"], blob=lambda n: z[f"jpeg_{names.index(n)}"].tobytes(), rgb=lambda n: z[f"rgb_{names.index(n)}"],
                blobs=[z[f"jpeg_{k}"].tobytes() for k in range(len(names))], z=z)


def images(buf, offsets, shapes):
    flat = buf.cpu().numpy()
    return [flat[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offsets, shapes)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_decode(eng, blobs, dst_bytes=None, dst_offsets=None):
    """mvlpt_jpeg_decode itself: (return code, destination tensor, offsets, status tensor)"""
    from mvlpt_amd import _lib, jpeg
    B = len(blobs)
    infos = [jpeg.probe(b) for b in blobs]
    sizes = [len(b) for b in blobs]
    src_off = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if B else []
    host = torch.from_numpy(np.frombuffer(b"".join(blobs) or b"\0", np.uint8).copy())
    dev = host.cuda()
    offsets, total = [], 0
    for f in infos:
        offsets.append(total)
        total += f.height * f.width * 3
    offsets = offsets if dst_offsets is None else dst_offsets
    dst = torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda")
    status = torch.full((max(B, 1),), 77, dtype=torch.int32, device="cuda")
    i64 = C.c_int64 * max(B, 1)
    rc = _lib.lib.mvlpt_jpeg_decode(eng.h, C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), i64(*src_off), i64(*sizes), B,
                                    C.c_void_p(dst.data_ptr()), total if dst_bytes is None else dst_bytes, i64(*offsets),
                                    C.c_void_p(status.data_ptr()), stream())
    torch.cuda.synchronize()
    return rc, dst, offsets, status, infos


def test_every_supported_fixture_equals_pillow(eng, golden):
    keep = [k for k, kind in enumerate(golden["kinds"]) if kind == 0]
    rc, dst, offsets, status, infos = raw_decode(eng, [golden["blobs"][k] for k in keep])
    assert rc == 0 and not status.cpu().numpy().any()
    got = images(dst, offsets, [(f.height, f.width) for f in infos])
    for k, g in zip(keep, got):
        assert np.array_equal(g, golden["z"][f"rgb_{k}"]), golden["names"][k]


STAGE_CASES = ["100x75_noise_420_q75rst5", "100x75_noise_422_q75rstrow", "37x45_noise_444_q100", "17x23_noise_gray_q100",
               "9x50_smooth_420_q30opt", "1x1_noise_420_q90", "100x75_smooth_420_q90"]


@pytest.mark.parametrize("name", STAGE_CASES)
def test_entropy_stage_equals_ref(golden, name):
    from mvlpt_amd import _lib
    blob = golden["blob"](name)
    P, coefs, _, _, st = jpeg_ref.decode_stages(blob)
    want = np.concatenate(coefs)
    host = torch.from_numpy(np.frombuffer(blob, np.uint8).copy())
    dev = host.cuda()
    ws = torch.empty(4096 + 8 * P.n_segments, dtype=torch.uint8, device="cuda")
    out = torch.full((want.shape[0], 64), 99, dtype=torch.int16, device="cuda")
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    args = [C.c_void_p(host.data_ptr()), len(blob), C.c_void_p(dev.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(out.data_ptr())]
    _lib.check(_lib.lib.mvlpt_op_jpeg_entropy(*args, want.shape[0], C.c_void_p(status.data_ptr()), stream()), None, "op_jpeg_entropy")
    torch.cuda.synchronize()
    assert int(status.cpu()) == st == 0 and np.array_equal(out.cpu().numpy(), want)
    assert _lib.lib.mvlpt_op_jpeg_entropy(*args, want.shape[0] + 1, C.c_void_p(status.data_ptr()), stream()) == _lib.ERR_ARG   # a wrong block count
    bad = torch.from_numpy(np.frombuffer(golden["blob"]("fallback_progressive"), np.uint8).copy())
    args[0], args[1] = C.c_void_p(bad.data_ptr()), bad.numel()
    assert _lib.lib.mvlpt_op_jpeg_entropy(*args, 1, C.c_void_p(status.data_ptr()), stream()) == _lib.ERR_UNSUPPORTED


def test_idct_stage_equals_ref_at_the_range_extremes():
    """Coefficients over the whole baseline range (quantised |DC| <= 2047, |AC| <= 1023), at quantisation 1 and 255: with 255 the
    products pass 2^31 inside the passes, where the device's unsigned wrap must equal the reference's wrap to 32 bits."""
    from mvlpt_amd import _lib
    rng = np.random.default_rng(5)
    n, bw = 70, 7                                                 # three workgroups of 32 blocks, the last one partial
    c = rng.integers(-1023, 1024, (n, 64)).astype(np.int16)
    c[:, 0] = rng.integers(-2047, 2048, n)
    c[0], c[1] = 1023, -1023
    c[0, 0], c[1, 0] = 2047, -2047
    c[2] = 0
    c[3] = 0
    c[3, 0] = -2047
    c[4] = np.where(np.arange(64) % 2, 1023, -1023)
    c[5, 1:] = 0                                                   # DC only
    c[6:40] = np.clip(c[6:40] // 64, -16, 16)                      # ordinary image-like magnitudes
    for q in (np.ones(64, np.uint8), np.full(64, 255, np.uint8), rng.integers(1, 256, 64).astype(np.uint8)):
        want = jpeg_ref.planes_from_blocks(jpeg_ref.idct_blocks(c, q), n // bw, bw)
        out = torch.zeros(n // bw * 8, bw * 8, dtype=torch.uint8, device="cuda")
        cd, qd = torch.from_numpy(c).cuda(), torch.from_numpy(q).cuda()
        _lib.check(_lib.lib.mvlpt_op_jpeg_idct(C.c_void_p(cd.data_ptr()), C.c_void_p(qd.data_ptr()), n, bw, C.c_void_p(out.data_ptr()), stream()),
                   None, "op_jpeg_idct")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), int(q[1])
    assert _lib.lib.mvlpt_op_jpeg_idct(C.c_void_p(cd.data_ptr()), C.c_void_p(qd.data_ptr()), n, 8, C.c_void_p(out.data_ptr()), stream()) == _lib.ERR_ARG


@pytest.mark.parametrize("width", [1, 2, 9, 37])
@pytest.mark.parametrize("sampling", [(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)])
def test_colour_stage_equals_ref(width, sampling):
    """planes 1, 2 and 9 samples wide (and 37: more than one group of four pixels per row, an odd tail), heights 1 .. 5"""
    from mvlpt_amd import _lib
    ncomp, hs, vs = sampling
    rng = np.random.default_rng(width * 10 + hs + vs)
    for H in (1, 2, 5):
        pw = [-(-width // 8) * 8 * (hs if c == 0 else 1) for c in range(ncomp)]
        ph = [-(-H // 8) * 8 * (vs if c == 0 else 1) for c in range(ncomp)]
        planes = [rng.integers(0, 256, (ph[c], pw[c])).astype(np.uint8) for c in range(ncomp)]
        want = jpeg_ref.colour(planes, width, H, hs, vs)
        flat = np.concatenate([p.reshape(-1) for p in planes])
        offs = np.concatenate([[0], np.cumsum([p.size for p in planes])[:-1]])
        pd = torch.from_numpy(flat).cuda()
        out = torch.full((H * width * 3 + 5,), 200, dtype=torch.uint8, device="cuda")
        for shift in (0, 1):                                       # an aligned and a misaligned destination
            _lib.check(_lib.lib.mvlpt_op_jpeg_colour(C.c_void_p(pd.data_ptr()), (C.c_int64 * 3)(*[int(v) for v in offs]), (C.c_int32 * 3)(*pw), ncomp,
                                                     hs, vs, H, width, C.c_void_p(out.data_ptr() + shift), stream()), None, "op_jpeg_colour")
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[shift:shift + H * width * 3].reshape(H, width, 3), want), (H, shift)
            assert (got[shift + H * width * 3:] == 200).all()      # nothing written behind the image


def test_mixed_batch_with_fallbacks(eng, golden):
    from mvlpt_amd import jpeg
    names = ["37x45_noise_444_q90", "fallback_progressive", "37x45_noise_422_q75rst1", "fallback_cmyk", "100x75_noise_420_q75rstrow",
             "17x23_smooth_gray_q30opt", "fallback_440", "1x1_smooth_420_q90"]
    buf, offsets, shapes, status = jpeg.decode_batch(eng, [golden["blob"](n) for n in names])
    assert status.cpu().tolist() == [-1 if n.startswith("fallback") else 0 for n in names]
    for n, g in zip(names, images(buf, offsets, shapes)):
        assert np.array_equal(g, golden["rgb"](n)), n


def test_malformed_files_among_good_neighbours(eng, golden):
    from mvlpt_amd import jpeg
    names = ["37x45_noise_420_q90", "malformed_cut", "16x33_noise_422_q90", "malformed_byte", "33x16_noise_gray_q75rst1"]
    blobs = [golden["blob"](n) for n in names]
    buf, offsets, shapes, status = jpeg.decode_batch(eng, blobs, check=False)
    st = status.cpu().tolist()
    assert st[0] == st[2] == st[4] == 0 and st[1] > 0 and st[3] > 0
    assert st[1] == jpeg_ref.decode(blobs[1])[1] and st[3] == jpeg_ref.decode(blobs[3])[1]
    got = images(buf, offsets, shapes)
    for k in (0, 2, 4):
        assert np.array_equal(got[k], golden["rgb"](names[k])), names[k]
    for k in (1, 3):                                               # the damaged data decodes to what the same arithmetic gives on the CPU
        assert np.array_equal(got[k], jpeg_ref.decode(blobs[k])[0]), names[k]
    buf, offsets, shapes, status = jpeg.decode_batch(eng, blobs, check=True)
    got = images(buf, offsets, shapes)
    for k, n in enumerate(names):
        try:
            want = np.asarray(Image.open(io.BytesIO(blobs[k])).convert("RGB"))
        except OSError:
            assert n == "malformed_cut"                            # Pillow refuses a truncated file
            continue
        assert np.array_equal(got[k], want), n


def test_two_calls_are_bit_equal_and_empty_batch(eng, golden):
    from mvlpt_amd import jpeg
    blobs = [golden["blob"](n) for n in ("100x75_noise_420_q75rst5", "37x45_noise_422_q100", "9x50_noise_444_q90")]
    a = jpeg.decode_batch(eng, blobs)
    b = jpeg.decode_batch(eng, blobs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    rc, _, _, status, _ = raw_decode(eng, [])
    assert rc == 0 and int(status.cpu()[0]) == 77                  # B == 0: nothing touched
    buf, offsets, shapes, status = jpeg.decode_batch(eng, [])
    assert buf.numel() == 0 and offsets == [] and shapes == [] and status.numel() == 0


def test_short_destination_is_refused_before_any_launch(eng, golden):
    from mvlpt_amd import _lib
    blobs = [golden["blob"]("37x45_noise_420_q90"), golden["blob"]("17x23_noise_444_q90")]
    total = (45 * 37 + 23 * 17) * 3
    rc, dst, _, status, _ = raw_decode(eng, blobs, dst_bytes=total - 1)
    assert rc == _lib.ERR_ARG and "does not fit" in _lib.last_error(eng.h)
    assert not dst.cpu().numpy().any() and status.cpu().tolist() == [77, 77]
    rc, *_ = raw_decode(eng, blobs, dst_offsets=[0, -4])
    assert rc == _lib.ERR_ARG
    rc, dst, offsets, status, infos = raw_decode(eng, blobs, dst_bytes=total)
    assert rc == 0 and status.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("kwargs", [dict(train=True), dict(train=False),
                                    dict(train=True, transforms=("random_crop", "random_flip", "colorjitter", "randomgrayscale", "cutout",
                                                                 "normalize"))])
def test_from_encoded_equals_call(eng, golden, kwargs):
    from mvlpt_amd.transforms import DeviceTransform
    names = ["100x75_noise_420_q75rstrow", "37x45_noise_422_q90", "fallback_progressive", "100x75_smooth_gray_q90", "33x16_noise_444_q30opt"]
    blobs = [golden["blob"](n) for n in names]
    arrays = [golden["rgb"](n) for n in names]
    a = DeviceTransform(eng, size=32, generator=torch.Generator().manual_seed(3), **kwargs)
    b = DeviceTransform(eng, size=32, generator=torch.Generator().manual_seed(3), **kwargs)
    out, u8 = a.from_encoded(blobs, want_u8=True)
    want, want_u8 = b(arrays, want_u8=True)
    assert torch.equal(u8, want_u8) and torch.equal(out, want)
