"""Device augmentations (`mvlpt_preprocess_aug`, csrc/preprocess.hip) through the C ABI, -m gpu.
Bar: BIT-EXACT (np.array_equal, no case excluded) -- the 8-bit image before ToTensor equals Pillow's (tests/golden/augment.npz) and
tests/augment_ref.py (held to Pillow by tests/test_augment_ref.py) on top of the C resample oracle; fp32 equals torch's
(u8 / 255 - mean) / std; f16 equals that fp32 value rounded once."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import augment_ref as R  # noqa: E402
from tests.augment_ref import golden_cases, reference_window  # noqa: E402
from tests.golden_util import load_npz  # noqa: E402

MEAN, STD = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)


@pytest.fixture(scope="module")
def eng():
    from mvlpt_amd.engine import Engine
    from mvlpt_amd.weights import ARCHS
    return Engine(ARCHS["tiny"], "fp16")


def item(src, crop=None, resize=None, origin=(0, 0), flip=0, ops=(), factor=(1.0, 1.0, 1.0), shift=0, gray=0, holes=()):
    h, w = src.shape[:2]
    crop = crop or (0, 0, h, w)
    return dict(src=src, crop=crop, resize=resize or (crop[2], crop[3]), origin=origin, flip=flip, ops=list(ops),
                factor=np.asarray(factor, np.float32), shift=shift, gray=gray, holes=list(holes))


def pack(items):
    """-> (packed uint8 device tensor, image descriptors, augmentation descriptors)"""
    from mvlpt_amd import _lib
    descs, augs = (_lib.MvlptImageDesc * len(items))(), (_lib.MvlptAugmentDesc * len(items))()
    off, chunks = 0, []
    for d, a, it in zip(descs, augs, items):
        s = it["src"]
        d.offset, d.height, d.width = off, s.shape[0], s.shape[1]
        d.crop_top, d.crop_left, d.crop_height, d.crop_width = it["crop"]
        (d.resize_height, d.resize_width), (d.out_top, d.out_left), d.flip = it["resize"], it["origin"], it["flip"]
        a.n_ops = len(it["ops"])
        a.ops[:min(a.n_ops, 4)] = it["ops"][:4]                        # a malformed n_ops = 5 keeps its count
        a.factor[:] = [float(v) for v in it["factor"]]
        a.hue_shift, a.grayscale, a.n_holes = it["shift"], it["gray"], len(it["holes"])
        for k, hole in enumerate(it["holes"]):
            a.hole[k][:] = hole
        off += s.size
        chunks.append(np.ascontiguousarray(s).reshape(-1))
    return torch.from_numpy(np.concatenate(chunks)).cuda(), descs, augs


def want_u8(it, out_hw):
    win = reference_window(it["src"], it["crop"], it["resize"], (*it["origin"], *out_hw), it["flip"])
    return R.chain(win, it["ops"], it["factor"], it["shift"], it["gray"], it["holes"])


def check(eng, items, out_hw, fill, mean=MEAN, std=STD, f16=False):
    src, descs, augs = pack(items)
    out, u8 = eng.preprocess_aug(src, descs, augs, out_hw, mean, std, torch.float32, want_u8=True, fill_outside=fill)
    out, u8 = out.cpu().numpy(), u8.cpu().numpy()
    out16 = eng.preprocess_aug(src, descs, augs, out_hw, mean, std, torch.float16, fill_outside=fill).cpu() if f16 else None
    for k, it in enumerate(items):
        w8 = it["want"] if "want" in it else want_u8(it, out_hw)
        assert np.array_equal(u8[k], w8), f"image {k}: bytes differ ({int((u8[k] != w8).any(-1).sum())} pixels)"
        w32 = R.to_tensor_normalize(w8, mean, std)
        assert np.array_equal(out[k], w32), f"image {k}: fp32 differs from (u8 / 255 - mean) / std"
        if f16:
            assert torch.equal(out16[k], torch.from_numpy(w32).half()), f"image {k}: f16 is not the fp32 value rounded once"
    return u8


def test_golden_chains_equal_pillow(eng):
    cases, mean, std = golden_cases()
    groups = {}
    for (src, crop, resize, window, flip, fill, ops, factor, shift, gray, holes, want) in cases:
        it = item(src, crop, resize, window[:2], flip, ops, factor, shift, gray, holes)
        it["want"] = want                                              # Pillow's bytes
        groups.setdefault((window[2], window[3], fill), []).append(it)
    assert len(groups) >= 4
    for (oh, ow, fill), items in groups.items():
        check(eng, items, (oh, ow), fill, mean, std, f16=True)
    # fp32 against torch itself on one case
    it = groups[(32, 32, 0)][0]
    src, descs, augs = pack([it])
    out = eng.preprocess_aug(src, descs, augs, 32, mean, std)
    t = torch.from_numpy(it["want"]).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    assert torch.equal(out[0].cpu(), (t - torch.from_numpy(mean)[:, None, None]) / torch.from_numpy(std)[:, None, None])


def _random_source(rng, k):
    H, W = int(rng.integers(1, 120)), int(rng.integers(1, 120))
    if k % 2:
        return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    return np.clip(np.add.outer(np.arange(H) * 2, np.arange(W) * 3)[..., None] % 256 + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8)


ORDERS = list(itertools.permutations(range(4)))


@pytest.mark.parametrize("kind,out_hw", [("orders", (32, 32)), ("lengths", (48, 48)), ("one_pixel", (1, 1)), ("odd", (33, 47))])
def test_ragged_batches_equal_the_reference(eng, kind, out_hw):
    """24 images of different sizes: every order of the four operations (`orders`), chains of length 0..4 (the other kinds), factors
    0, exactly 1, inside (0, 1) and above 1, hue shifts 0 / 1 / 128 / 255, grayscale and flip on and off."""
    rng = np.random.default_rng(["orders", "lengths", "one_pixel", "odd"].index(kind))
    items = []
    for k in range(24):
        a = _random_source(rng, k)
        H, W = a.shape[:2]
        ch, cw = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        ct, cl = int(rng.integers(0, H - ch + 1)), int(rng.integers(0, W - cw + 1))
        if k % 5 == 0:                                                 # a window inside a larger resized image
            rh, rw = out_hw[0] + int(rng.integers(0, 20)), out_hw[1] + int(rng.integers(0, 20))
            origin = (int(rng.integers(0, rh - out_hw[0] + 1)), int(rng.integers(0, rw - out_hw[1] + 1)))
        else:
            (rh, rw), origin = out_hw, (0, 0)
        ops = ORDERS[k] if kind == "orders" else ORDERS[(7 * k) % 24][:k % 5]
        pool = [0.0, 1.0, float(rng.uniform(0.05, 0.95)), float(rng.uniform(1.05, 2.0))]
        factor = [pool[(k + j) % 4] for j in range(3)]
        items.append(item(a, (ct, cl, ch, cw), (rh, rw), origin, (k // 2) % 2, ops, factor, [0, 1, 128, 255][(k // 3) % 4], k % 2))
    assert kind != "orders" or sorted(tuple(it["ops"]) for it in items) == sorted(ORDERS)
    assert kind == "orders" or {len(it["ops"]) for it in items} == {0, 1, 2, 3, 4}
    check(eng, items, out_hw, fill=0, f16=(kind == "odd"))


@pytest.fixture(scope="module")
def lattice():
    """Four 512 x 512 windows: window o holds every triple of {4k + o}^3 -- every channel level, max == min, the ties of the hue branch."""
    v = np.arange(64, dtype=np.uint8) * 4
    base = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(512, 512, 3)
    return [base + np.uint8(o) for o in range(4)]


@pytest.mark.parametrize("name,ops,factor,shift,gray", [
    ("brightness", [0], (0.63, 1, 1), 0, 0), ("brightness_up", [0], (1.7, 1, 1), 0, 0),
    ("contrast", [1], (1, 0.45, 1), 0, 0), ("contrast_up", [1], (1, 1.6, 1), 0, 0),
    ("saturation", [2], (1, 1, 0.3), 0, 0), ("saturation_up", [2], (1, 1, 1.9), 0, 0),
    ("hue_0", [3], (1, 1, 1), 0, 0), ("hue_77", [3], (1, 1, 1), 77, 0), ("grayscale", [], (1, 1, 1), 0, 1)])
def test_colour_lattice_through_identity_resample(eng, lattice, name, ops, factor, shift, gray):
    items = [item(a, ops=ops, factor=factor, shift=shift, gray=gray) for a in lattice]
    src, descs, augs = pack(items)
    _, u8 = eng.preprocess_aug(src, descs, augs, 512, MEAN, STD, torch.float16, want_u8=True)
    u8 = u8.cpu().numpy()
    for o, it in enumerate(items):
        want = R.chain(it["src"], it["ops"], it["factor"], shift, gray)
        assert np.array_equal(u8[o], want), f"{name}, lattice offset {o}: {int((u8[o] != want).any(-1).sum())} pixels differ"


def test_fill_outside_windows(eng):
    """A window over each side, over two opposite sides at once, and wholly outside; with and without flip; behind a skipped (identity)
    pass and a real resample; every other image with a contrast operation, whose mean counts the padding."""
    rng = np.random.default_rng(7)
    R_ = 32
    # (resized size, window origin)
    geoms = [((32, 32), (-5, 0)), ((32, 32), (6, 0)), ((32, 32), (0, -7)), ((32, 32), (2, 9)),        # top, bottom, left, right
             ((20, 40), (-6, 3)), ((40, 18), (4, -8)),                                               # top + bottom, left + right
             ((32, 32), (-32, 0)), ((32, 32), (0, 32)), ((32, 32), (40, -50))]                      # wholly outside
    items = []
    for n, ((rh, rw), origin) in enumerate(geoms):
        for flip in (0, 1):
            for real in (0, 1):
                src = rng.integers(0, 256, ((rh + 9, rw + 5) if real else (rh, rw)) + (3,)).astype(np.uint8)
                ops, factor = ([1], (1, 0.5, 1)) if (n + flip + real) % 2 else ([], (1, 1, 1))
                items.append(item(src, None, (rh, rw), origin, flip, ops, factor))
    u8 = check(eng, items, (R_, R_), fill=1)
    assert (u8[-12:] == 0).all() and (u8[:8] != 0).any()
    # fill_outside with no augmentation descriptors at all (random_crop with padding alone)
    src, descs, _ = pack(items)
    _, plain = eng.preprocess_aug(src, descs, None, R_, MEAN, STD, want_u8=True, fill_outside=True)
    for k, it in enumerate(items):
        assert np.array_equal(plain[k].cpu().numpy(), reference_window(it["src"], it["crop"], it["resize"], (*it["origin"], R_, R_), it["flip"]))


def test_holes(eng):
    rng = np.random.default_rng(8)
    holes = [[], [(0, 0, 32, 32)], [(0, 0, 1, 1)], [(31, 31, 1, 1), (0, 31, 5, 1)], [(4, 4, 16, 16), (12, 12, 16, 16)],
             [(0, 10, 32, 3), (10, 0, 3, 32), (28, 0, 4, 32)], [(0, 0, 8, 8), (0, 24, 8, 8), (24, 0, 8, 8), (24, 24, 8, 8)],
             [(5, 5, 10, 10), (5, 5, 10, 10), (6, 6, 2, 2), (14, 14, 18, 18)]]
    items = [item(rng.integers(1, 256, (40 + k, 50 - k, 3)).astype(np.uint8), None, (32, 32), (0, 0), k % 2,
                  [2, 0][:k % 3], (1.2, 1, 0.5), 0, int(k == 5), h) for k, h in enumerate(holes)]
    u8 = check(eng, items, (32, 32), fill=0)
    assert (u8[1] == 0).all() and (u8[0] != 0).any() and (u8[6][:8, :8] == 0).all() and (u8[6][8:24] != 0).any()


def test_plain_call_is_mvlpt_preprocess(eng):
    """aug = NULL, fill_outside = 0: the same bits as `mvlpt_preprocess` on its own golden, every output dtype."""
    g = load_npz("preprocess")
    by_size = {}
    for i in range(int(g["n"])):
        ct, cl, ch, cw, rh, rw, ot, ol, oh, ow, flip = [int(v) for v in g[f"c{i}_desc"]]
        by_size.setdefault((oh, ow), []).append((i, item(g[f"c{i}_src"], (ct, cl, ch, cw), (rh, rw), (ot, ol), flip)))
    for (oh, ow), cases in by_size.items():
        src, descs, _ = pack([c for _, c in cases])
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            a, a8 = eng.preprocess(src, descs, (oh, ow), g["mean"], g["std"], dt, want_u8=True)
            b, b8 = eng.preprocess_aug(src, descs, None, (oh, ow), g["mean"], g["std"], dt, want_u8=True)
            assert torch.equal(a, b) and torch.equal(a8, b8)
        for k, (i, _) in enumerate(cases):
            assert np.array_equal(b8[k].cpu().numpy(), g[f"c{i}_u8"])
        # and the augmented route with nothing to do computes the same again
        c, c8 = eng.preprocess_aug(src, descs, None, (oh, ow), g["mean"], g["std"], torch.bfloat16, want_u8=True, fill_outside=True)
        assert torch.equal(b, c) and torch.equal(b8, c8)


def test_deterministic_and_contrast_uses_each_images_own_mean(eng):
    rng = np.random.default_rng(9)
    dark, bright = rng.integers(0, 60, (32, 32, 3)).astype(np.uint8), rng.integers(180, 256, (32, 32, 3)).astype(np.uint8)
    items = [item(dark, ops=[1], factor=(1, 0.0, 1)), item(bright, ops=[1], factor=(1, 0.0, 1)),
             item(dark, ops=[3, 1, 2], factor=(1, 1.4, 0.7), shift=9), item(bright, ops=[0, 1], factor=(0.5, 0.3, 1))]
    u8 = check(eng, items, (32, 32), fill=0)
    assert (u8[0] == R.contrast_mean(dark)).all() and (u8[1] == R.contrast_mean(bright)).all() and u8[0][0, 0, 0] != u8[1][0, 0, 0]
    src, descs, augs = pack(items)
    a = eng.preprocess_aug(src, descs, augs, 32, MEAN, STD, want_u8=True)
    b = eng.preprocess_aug(src, descs, augs, 32, MEAN, STD, want_u8=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_malformed_descriptors_leave_the_outputs_untouched(eng):
    from mvlpt_amd import _lib
    src_a = np.full((32, 32, 3), 200, np.uint8)
    good = item(src_a, ops=[0, 3], factor=(1.5, 1, 1), shift=5, holes=[(0, 0, 4, 4)])
    bad = [dict(ops=[0, 2, 0]), dict(ops=[0, 1, 2, 3, 0]), dict(ops=[1], factor=(1, float("nan"), 1)), dict(ops=[2], factor=(1, 1, -0.5)),
           dict(ops=[0], factor=(float("inf"), 1, 1)), dict(ops=[4]), dict(ops=[3], shift=256), dict(holes=[(30, 0, 4, 4)]),
           dict(holes=[(0, -1, 4, 4)]), dict(holes=[(0, 0, 0, 4)]), dict(origin=(1, 0)), dict(origin=(0, -1)), dict(gray=2)]
    out = torch.full((2, 3, 32, 32), 7.0, device="cuda")
    u8 = torch.full((2, 32, 32, 3), 9, dtype=torch.uint8, device="cuda")
    m, sd = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)

    def call(items, n_ops=None, n_holes=None, fill=0, B=None):
        src, descs, augs = pack(items)
        if n_ops is not None:
            augs[1].n_ops = n_ops
        if n_holes is not None:
            augs[1].n_holes = n_holes
        rc = _lib.lib.mvlpt_preprocess_aug(eng.h, src.data_ptr(), src.numel(), descs, augs, len(items) if B is None else B, 32, 32, fill, m,
                                           sd, out.data_ptr(), _lib.DT_F32, u8.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    for kw in bad:
        it = dict(good, **{k: (np.asarray(v, np.float32) if k == "factor" else v) for k, v in kw.items()})
        assert call([good, it]) == _lib.ERR_ARG, kw
        assert "1" in _lib.last_error(eng.h)
    assert call([good, good], n_ops=5) == _lib.ERR_ARG and call([good, good], n_ops=-1) == _lib.ERR_ARG
    assert call([good, good], n_holes=5) == _lib.ERR_ARG and call([good, good], fill=2) == _lib.ERR_ARG
    assert call([good, good], B=-1) == _lib.ERR_ARG
    assert (out == 7.0).all() and (u8 == 9).all()                     # nothing was launched
    assert call([good, good], B=0) == 0 and (out == 7.0).all() and (u8 == 9).all()
    assert call([good, dict(good, origin=(1, 0))], fill=1) == 0       # the same window is fine with fill_outside
    assert call([good, good]) == 0 and not (u8 == 9).all()
    assert eng.preprocess_aug(torch.zeros(0, dtype=torch.uint8, device="cuda"), (_lib.MvlptImageDesc * 0)(), None, 32, MEAN, STD).shape == (0, 3, 32, 32)
    with pytest.raises(RuntimeError, match="augmentation 0"):
        src, descs, augs = pack([dict(good, ops=[1, 1])])
        eng.preprocess_aug(src, descs, augs, 32, MEAN, STD)
    with pytest.raises(RuntimeError, match="no CPU path"):
        eng.preprocess_aug(src.cpu(), descs, augs, 32, MEAN, STD)


def test_device_transform_with_dassls_names(eng):
    """build_device_transform end to end: the batch equals the reference applied to the descriptors an equally seeded transform draws."""
    from mvlpt_amd.config import get_cfg_default
    from mvlpt_amd.transforms import CLIP_MEAN, CLIP_STD, build_device_transform
    rng = np.random.default_rng(10)
    imgs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in [(60, 80), (80, 60), (32, 32), (25, 100), (47, 33), (90, 90)]]
    for names in (["random_crop", "random_flip", "colorjitter", "randomgrayscale", "cutout", "normalize"],
                  ["random_resized_crop", "colorjitter", "cutout"], ["center_crop", "randomgrayscale", "normalize"], ["random_crop"]):
        cfg = get_cfg_default()
        cfg.INPUT.SIZE, cfg.INPUT.TRANSFORMS, cfg.INPUT.RGS_P, cfg.INPUT.CUTOUT_N = (32, 32), names, 0.5, 2
        tr = build_device_transform(cfg, eng, generator=torch.Generator().manual_seed(21))
        descs, augs, _ = build_device_transform(cfg, eng, generator=torch.Generator().manual_seed(21)).describe_aug([im.shape[:2] for im in imgs])
        out, u8 = tr(imgs, want_u8=True)
        mean, std = (CLIP_MEAN, CLIP_STD) if "normalize" in names else ((0, 0, 0), (1, 1, 1))
        for k, (im, d) in enumerate(zip(imgs, descs)):
            win = reference_window(im, (d.crop_top, d.crop_left, d.crop_height, d.crop_width), (d.resize_height, d.resize_width),
                                   (d.out_top, d.out_left, 32, 32), d.flip)
            if augs is not None:
                a = augs[k]
                win = R.chain(win, a.ops[:a.n_ops], a.factor[:], a.hue_shift, a.grayscale, [tuple(h) for h in a.hole[:a.n_holes]])
            assert np.array_equal(u8[k].cpu().numpy(), win), (names, k)
            assert np.array_equal(out[k].cpu().numpy(), R.to_tensor_normalize(win, mean, std)), (names, k)
