"""tests/augment_ref.py (the numpy restatement the device augmentations are held to) against Pillow itself: every primitive on
random images, both HSV conversions on all 2^24 triples, whole chains against tests/golden/augment.npz (made by
tools/make_augment_golden.py with Pillow alone).  And the host side of mvlpt_amd.transforms: the default DeviceTransform draws what
it drew before, build_device_transform reads Dassl's names and composes them in Dassl's fixed order.  Bar: np.array_equal."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.augment_ref import golden_cases, reference_window


def test_primitives_equal_pillow_on_random_images():
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(0)
    for k in range(200):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8) if k % 3 else (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        im = Image.fromarray(a)
        f = float(np.float32([0.0, 1.0, rng.uniform(0, 1), rng.uniform(1, 2)][k % 4]))
        assert np.array_equal(np.asarray(im.convert("L")), R.luma(a))
        assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(f)), R.brightness(a, f)), f
        assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), R.saturation(a, f)), f
        assert np.array_equal(np.asarray(ImageEnhance.Contrast(im).enhance(f)), R.contrast(a, f)), f
        assert np.array_equal(np.asarray(im.convert("HSV")), R.rgb_to_hsv(a))
        assert np.array_equal(np.asarray(Image.frombytes("HSV", (w, h), a.tobytes()).convert("RGB")), R.hsv_to_rgb(a))


def test_hsv_conversions_equal_pillow_on_the_full_cube():
    from PIL import Image
    v = np.arange(256, dtype=np.uint8)
    for r in range(0, 256, 16):
        cube = np.stack(np.meshgrid(v[r:r + 16], v, v, indexing="ij"), -1).reshape(16 * 256, 256, 3)
        assert np.array_equal(np.asarray(Image.fromarray(cube).convert("HSV")), R.rgb_to_hsv(cube)), r
        assert np.array_equal(np.asarray(Image.frombytes("HSV", (256, 4096), cube.tobytes()).convert("RGB")), R.hsv_to_rgb(cube)), r


def test_hue_round_trip_is_not_the_identity():
    a = np.random.default_rng(2).integers(0, 256, (64, 64, 3)).astype(np.uint8)
    a[0] = a[0, :, :1]                                       # a grey row: S == 0 comes back as it was
    out = R.hue(a, 0)
    assert (out != a).any(-1).mean() > 0.1 and np.array_equal(out[0], a[0])


def test_chains_equal_the_golden():
    cases, _, _ = golden_cases()
    assert len(cases) >= 12 and any(c[5] for c in cases) and any(len(c[6]) == 4 for c in cases)
    for i, (src, crop, resize, window, flip, fill, ops, factor, shift, gray, holes, want) in enumerate(cases):
        got = R.chain(reference_window(src, crop, resize, window, flip), ops, factor, shift, gray, holes)
        assert np.array_equal(got, want), f"case {i}"


def test_to_tensor_normalize_equals_torch():
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, (9, 7, 3)).astype(np.uint8)
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    want = (t - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
    assert np.array_equal(R.to_tensor_normalize(u8, mean, std), want.numpy())


# ------------------------------------------------------------------------------------------------ host side (no GPU)
SHAPES = [(375, 500), (500, 375), (64, 64), (300, 1000), (1, 50)]


def _fields(descs):
    return [tuple(getattr(d, n) for n, _ in d._fields_) for d in descs]


def _augs(augs):
    return [(a.n_ops, tuple(a.ops), tuple(a.factor), a.hue_shift, a.grayscale, a.n_holes, tuple(tuple(h) for h in a.hole)) for a in augs]


def test_default_transform_draws_what_it_drew_before():
    """The draws of the three-transform pipeline, restated: RandomResizedCrop.get_params, then one uniform for the flip."""
    from mvlpt_amd.transforms import DeviceTransform, random_resized_crop_params
    for seed in (0, 5):
        g = torch.Generator().manual_seed(seed)
        want, off = [], 0
        for (h, w) in SHAPES:
            box = random_resized_crop_params(h, w, generator=g)
            flip = int(float(torch.rand(1, generator=g)) < 0.5)
            want.append((off, h, w, *box, 224, 224, 0, 0, flip, 0))
            off += h * w * 3
        tr = DeviceTransform(engine=None, size=224, train=True, generator=torch.Generator().manual_seed(seed))
        descs, augs, total = tr.describe_aug(SHAPES)
        assert _fields(descs) == want and total == off and augs is None and not tr.fill_outside
        again = DeviceTransform(engine=None, size=224, train=True, generator=torch.Generator().manual_seed(seed),
                                transforms=["normalize", "random_flip", "random_resized_crop"]).describe(SHAPES)
        assert _fields(again[0]) == want and again[1] == off


def _cfg(names, **over):
    from mvlpt_amd.config import get_cfg_default
    cfg = get_cfg_default()
    cfg.INPUT.SIZE = (32, 32)
    cfg.INPUT.TRANSFORMS = list(names)
    for k, v in over.items():
        cfg.INPUT[k] = v
    return cfg


def test_config_carries_dassls_names_and_defaults():
    from mvlpt_amd.config import get_cfg_default
    inp = get_cfg_default().INPUT
    assert inp.TRANSFORMS == ["random_resized_crop", "random_flip", "normalize"]
    assert (inp.COLORJITTER_B, inp.COLORJITTER_C, inp.COLORJITTER_S, inp.COLORJITTER_H) == (0.4, 0.4, 0.4, 0.1)
    assert (inp.RGS_P, inp.CROP_PADDING, inp.CUTOUT_N, inp.CUTOUT_LEN) == (0.2, 4, 1, 16)
    cfg = get_cfg_default()
    cfg.merge_from_list(["INPUT.TRANSFORMS", '["random_crop", "cutout"]', "INPUT.CUTOUT_LEN", "8", "INPUT.RGS_P", "0.5"])
    assert cfg.INPUT.TRANSFORMS == ["random_crop", "cutout"] and cfg.INPUT.CUTOUT_LEN == 8 and cfg.INPUT.RGS_P == 0.5


def test_build_device_transform_names():
    from mvlpt_amd.transforms import ACCEPTED_TRANSFORMS, build_device_transform
    assert set(ACCEPTED_TRANSFORMS) == {"random_resized_crop", "random_crop", "random_flip", "center_crop", "colorjitter",
                                        "randomgrayscale", "cutout", "normalize"}
    for name in ACCEPTED_TRANSFORMS:
        build_device_transform(_cfg([name]), None, train=True)
    for bad in ("gaussian_blur", "gaussian_noise", "randaugment", "randaugment2", "randaugment_fixmatch", "imagenet_policy",
                "cifar10_policy", "svhn_policy", "random_translation", "instance_norm", "no_such_transform"):
        for train in (True, False):
            with pytest.raises(ValueError, match="accepted: .*colorjitter.*cutout"):
                build_device_transform(_cfg(["random_flip", bad]), None, train=train)
    with pytest.raises(ValueError, match="exclude one another"):
        build_device_transform(_cfg(["random_crop", "random_resized_crop"]), None)
    with pytest.raises(ValueError, match="cutout_n"):
        build_device_transform(_cfg(["cutout"], CUTOUT_N=5), None)
    # the default list is the present pipeline; testing is Resize + CenterCrop + normalize whatever the training list says
    tr = build_device_transform(_cfg(["random_resized_crop", "random_flip", "normalize"]), None)
    assert not tr.augments and not tr.fill_outside and tr.size == 32
    ev = build_device_transform(_cfg(["colorjitter", "random_crop", "cutout"]), None, train=False)
    descs, augs, _ = ev.describe_aug(SHAPES[:3])
    assert augs is None and not ev.fill_outside and all(d.flip == 0 and min(d.resize_height, d.resize_width) == 32 for d in descs)
    # without normalize Dassl adds no Normalize
    assert build_device_transform(_cfg(["random_flip"]), None).std == (1.0, 1.0, 1.0)


def test_composition_order_is_fixed_and_the_draws_are_in_range():
    from mvlpt_amd.transforms import build_device_transform
    names = ["random_crop", "random_flip", "colorjitter", "randomgrayscale", "cutout", "normalize"]
    shapes = SHAPES * 8
    ref = None
    for order in (names, names[::-1], names[3:] + names[:3]):
        tr = build_device_transform(_cfg(order, CUTOUT_N=3, RGS_P=0.5), None, generator=torch.Generator().manual_seed(3))
        descs, augs, _ = tr.describe_aug(shapes)
        got = (_fields(descs), _augs(augs))
        ref = ref or got
        assert got == ref and tr.fill_outside and tr.augments
    seen_ops, seen_gray, seen_off = set(), set(), set()
    for d, a in zip(descs, augs):
        assert (d.crop_top, d.crop_left, d.crop_height, d.crop_width) == (0, 0, d.height, d.width)
        assert d.resize_height == d.resize_width == 32 and -4 <= d.out_top <= 4 and -4 <= d.out_left <= 4
        ops = tuple(a.ops[:a.n_ops])
        assert sorted(ops) == [0, 1, 2, 3] and 0 <= a.hue_shift <= 255 and (a.hue_shift <= 25 or a.hue_shift >= 231)
        assert all(np.float32(0.6) <= f <= np.float32(1.4) for f in a.factor)
        assert 1 <= a.n_holes <= 3
        for t, l, h, w in (tuple(r) for r in a.hole[:a.n_holes]):
            assert 0 <= t and 0 <= l and 1 <= h <= 16 and 1 <= w <= 16 and t + h <= 32 and l + w <= 32
        seen_ops.add(ops), seen_gray.add(a.grayscale), seen_off.add((d.out_top, d.out_left))
    assert len(seen_ops) > 5 and seen_gray == {0, 1} and len(seen_off) > 10
    # a parameter of 0 leaves its operation out; with all four at 0 nothing is left
    tr = build_device_transform(_cfg(["colorjitter"], COLORJITTER_C=0.0, COLORJITTER_H=0.0), None, generator=torch.Generator().manual_seed(1))
    _, augs, _ = tr.describe_aug(SHAPES)
    assert all(sorted(a.ops[:a.n_ops]) == [0, 2] and a.hue_shift == 0 and a.factor[1] == 1.0 for a in augs)
