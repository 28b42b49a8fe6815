"""Host side of the device input pipeline: the transform the reference builds with Dassl's `build_transform`
(INPUT.TRANSFORMS = random_resized_crop / random_flip / normalize, bicubic, CLIP mean/std:
configs/trainers/MVLPT/vit_b16.yaml:8-13) and the ELEVATER eval transform (Resize(BICUBIC) [+ CenterCrop] + ToTensor +
Normalize: trainers/vision_benchmark/evaluation/feature.py:538-553), re-cut for a GPU: the host only draws the random
parameters and packs decoded uint8 images into one pinned buffer; crop, antialiased bicubic resample, flip, ToTensor
and Normalize run in `mvlpt_preprocess` (csrc/preprocess.hip), bit-identical to Pillow + torch CPU.

The launcher's `--transforms` reaches the same `build_transform`, so `DeviceTransform(transforms=...)` /
`build_device_transform` also take Dassl's `random_crop` (zero padding), `center_crop`, `colorjitter`, `randomgrayscale` and
`cutout`; their pixels run in `mvlpt_preprocess_aug`, bit-identical to Pillow's ImageEnhance / convert("L") / convert("HSV").

The parameter sampling follows torchvision's documented algorithms (`RandomResizedCrop.get_params`, `Resize` with an
int size, `CenterCrop`, `RandomCrop.get_params`, `ColorJitter.get_params`, `RandomGrayscale`) and Dassl's `Cutout`; neither
package is installed in the build image, so those few formulas and the order of the draws are restated from their
documentation and are NOT pinned against them — the pixel arithmetic (Pillow) is, by tests/golden/preprocess.npz and
tests/golden/augment.npz."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def random_resized_crop_params(height: int, width: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                               generator: Optional[torch.Generator] = None) -> Tuple[int, int, int, int]:
    """(top, left, h, w) as torchvision.transforms.RandomResizedCrop.get_params: 10 attempts at a box of random area
    fraction and log-uniform aspect ratio, then a centre crop clamped to the ratio range."""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = area * float(torch.empty(1).uniform_(scale[0], scale[1], generator=generator))
        aspect = math.exp(float(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            i = int(torch.randint(0, height - h + 1, (1,), generator=generator))
            j = int(torch.randint(0, width - w + 1, (1,), generator=generator))
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def resize_shorter_side(height: int, width: int, size: int) -> Tuple[int, int]:
    """Output (h, w) of torchvision `Resize(int)`: shorter side -> size, longer side int(size * long / short)."""
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def center_crop_offsets(height: int, width: int, out_h: int, out_w: int) -> Tuple[int, int]:
    """(top, left) of torchvision `CenterCrop` (Python round = round-half-even)."""
    if out_h > height or out_w > width:
        raise ValueError("CenterCrop larger than the resized image (padding) is not supported")
    return int(round((height - out_h) / 2.0)), int(round((width - out_w) / 2.0))


DEFAULT_TRANSFORMS = ("random_resized_crop", "random_flip", "normalize")
# the names of Dassl's build_transform that run on the device.  Not offered: gaussian_blur, gaussian_noise,
# random_translation, instance_norm and the randaugment / policy families.
ACCEPTED_TRANSFORMS = ("random_resized_crop", "random_crop", "random_flip", "center_crop", "colorjitter", "randomgrayscale", "cutout",
                       "normalize")


def check_transforms(names: Sequence[str]) -> Tuple[str, ...]:
    names = tuple(names)
    bad = [n for n in names if n not in ACCEPTED_TRANSFORMS]
    if bad:
        raise ValueError(f"transforms {bad} do not run on the device; accepted: {', '.join(ACCEPTED_TRANSFORMS)}")
    # one resample per image: a random_resized_crop OF a padded crop, or either of a centre crop, would need a second one
    if sum(n in names for n in ("random_resized_crop", "random_crop", "center_crop")) > 1:
        raise ValueError("random_resized_crop, random_crop and center_crop exclude one another on the device (one resample per image)")
    return names


def color_jitter_params(brightness: float, contrast: float, saturation: float, hue: float, generator: Optional[torch.Generator] = None):
    """(ops, factors, hue_shift) as torchvision.transforms.ColorJitter.get_params draws them: a random order of the four operations,
    then brightness / contrast / saturation factors uniform in [max(0, 1 - x), 1 + x] and the hue in [-h, h]; a parameter of 0 leaves its
    operation out.  hue_shift is what adjust_hue adds to the 8-bit H channel: trunc(hue * 255) modulo 256."""
    order = [int(k) for k in torch.randperm(4, generator=generator)]
    factors = [1.0, 1.0, 1.0]
    for k, x in enumerate((brightness, contrast, saturation)):
        if x:
            factors[k] = float(torch.empty(1).uniform_(max(0.0, 1.0 - x), 1.0 + x, generator=generator))
    shift = int(float(torch.empty(1).uniform_(-hue, hue, generator=generator)) * 255) % 256 if hue else 0
    on = (bool(brightness), bool(contrast), bool(saturation), bool(hue))
    return [k for k in order if on[k]], factors, shift


def cutout_holes(height: int, width: int, n_holes: int, length: int, generator: Optional[torch.Generator] = None):
    """(top, left, h, w) of Dassl's Cutout: centres uniform over the image, [c - length // 2, c + length // 2) clipped to it; empty
    rectangles are dropped."""
    holes = []
    for _ in range(n_holes):
        cy = int(torch.randint(0, height, (1,), generator=generator))
        cx = int(torch.randint(0, width, (1,), generator=generator))
        y1, y2 = max(cy - length // 2, 0), min(cy + length // 2, height)
        x1, x2 = max(cx - length // 2, 0), min(cx + length // 2, width)
        if y2 > y1 and x2 > x1:
            holes.append((y1, x1, y2 - y1, x2 - x1))
    return holes


class DeviceTransform:
    """train=True : `transforms`, Dassl's names (default random_resized_crop + random_flip + normalize, vit_b16.yaml:8-13), composed in
                 Dassl's fixed order whatever the order of the list: Resize((size, size)) unless random_resized_crop [Resize(size) +
                 CenterCrop(size) with center_crop] -> random_crop (pad `crop_padding` zeros, crop at a uniform offset) ->
                 random_resized_crop -> random_flip -> colorjitter -> randomgrayscale -> ToTensor -> cutout -> normalize.
    train=False: Resize(size) + CenterCrop(size) + normalize when `center_crop`, else Resize((size, size)) + normalize
                 (feature.py:538-553).
    Call with a list of decoded uint8 HWC numpy arrays (or uint8 tensors); returns the [B,3,size,size] device batch."""

    def __init__(self, engine, size: int = 224, train: bool = True, center_crop: bool = True, mean: Sequence[float] = CLIP_MEAN,
                 std: Sequence[float] = CLIP_STD, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p: float = 0.5,
                 out_dtype=torch.float32, generator: Optional[torch.Generator] = None, transforms: Optional[Sequence[str]] = None,
                 colorjitter=(0.4, 0.4, 0.4, 0.1), rgs_p: float = 0.2, crop_padding: int = 4, cutout_n: int = 1, cutout_len: int = 16):
        self.engine, self.size, self.train, self.center_crop = engine, int(size), train, center_crop
        self.mean, self.std, self.scale, self.ratio, self.flip_p = tuple(mean), tuple(std), scale, ratio, flip_p
        self.out_dtype, self.generator = out_dtype, generator
        self.transforms = check_transforms(DEFAULT_TRANSFORMS if transforms is None else transforms)
        self.colorjitter, self.rgs_p, self.crop_padding = tuple(float(v) for v in colorjitter), float(rgs_p), int(crop_padding)
        self.cutout_n, self.cutout_len = int(cutout_n), int(cutout_len)
        if len(self.colorjitter) != 4 or min(self.colorjitter) < 0 or self.colorjitter[3] > 0.5:
            raise ValueError("colorjitter is (brightness, contrast, saturation, hue), each >= 0 and hue <= 0.5")
        if self.crop_padding < 0 or not 0 <= self.cutout_n <= _lib.AUG_MAX_HOLES or self.cutout_len < 0:
            raise ValueError(f"crop_padding and cutout_len must be >= 0 and cutout_n in 0..{_lib.AUG_MAX_HOLES}")
        if train and "normalize" not in self.transforms:               # Dassl then adds no Normalize: (x - 0) / 1 == x in fp32
            self.mean, self.std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        # the window hangs over the resized image (zero filled) only under random_crop with padding
        self.fill_outside = train and "random_crop" in self.transforms and self.crop_padding > 0
        self.augments = train and any(n in self.transforms for n in ("colorjitter", "randomgrayscale", "cutout"))
        # ring of pinned staging buffers, each guarded by the event of its last H2D copy: the train step does not
        # synchronise per step, so the copy of batch i may still be queued when batch i+1 is packed
        self._ring: List[list] = [[None, None] for _ in range(3)]      # [pinned tensor, torch.cuda.Event]
        self._slot = -1

    def describe(self, shapes: Sequence[Tuple[int, int]]):
        """Descriptors (ctypes array) for images of the given (height, width); draws the random parameters."""
        descs, _, off = self.describe_aug(shapes)
        return descs, off

    def describe_aug(self, shapes: Sequence[Tuple[int, int]]):
        """(image descriptors, augmentation descriptors or None when no transform needs them, total source bytes).  Per image the draws
        come in the order of the composition: crop, flip, colorjitter, randomgrayscale, cutout."""
        R, names, g = self.size, self.transforms, self.generator
        descs = (_lib.MvlptImageDesc * len(shapes))()
        augs = (_lib.MvlptAugmentDesc * len(shapes))() if self.augments else None
        off = 0
        for k, (d, (h, w)) in enumerate(zip(descs, shapes)):
            d.offset, d.height, d.width = off, h, w
            off += h * w * 3
            if self.train:
                d.resize_height = d.resize_width = R
                d.out_top = d.out_left = 0
                if "random_resized_crop" in names:
                    d.crop_top, d.crop_left, d.crop_height, d.crop_width = random_resized_crop_params(h, w, self.scale, self.ratio, g)
                else:
                    d.crop_top = d.crop_left = 0
                    d.crop_height, d.crop_width = h, w
                    if "center_crop" in names:
                        d.resize_height, d.resize_width = resize_shorter_side(h, w, R)
                        d.out_top, d.out_left = center_crop_offsets(d.resize_height, d.resize_width, R, R)
                    elif "random_crop" in names:                       # RandomCrop.get_params on the padded image
                        p = self.crop_padding
                        d.out_top = int(torch.randint(0, 2 * p + 1, (1,), generator=g)) - p
                        d.out_left = int(torch.randint(0, 2 * p + 1, (1,), generator=g)) - p
                d.flip = int(float(torch.rand(1, generator=g)) < self.flip_p) if "random_flip" in names else 0
                if augs is None:
                    continue
                a = augs[k]
                if "colorjitter" in names:
                    ops, factors, a.hue_shift = color_jitter_params(*self.colorjitter, generator=g)
                    a.n_ops = len(ops)
                    a.ops[:len(ops)] = ops
                    a.factor[:] = factors
                if "randomgrayscale" in names:
                    a.grayscale = int(float(torch.rand(1, generator=g)) < self.rgs_p)
                if "cutout" in names:
                    holes = cutout_holes(R, R, self.cutout_n, self.cutout_len, g)
                    a.n_holes = len(holes)
                    for j, hole in enumerate(holes):
                        a.hole[j][:] = hole
            else:
                d.crop_top = d.crop_left = 0
                d.crop_height, d.crop_width = h, w
                if self.center_crop:
                    d.resize_height, d.resize_width = resize_shorter_side(h, w, R)
                    d.out_top, d.out_left = center_crop_offsets(d.resize_height, d.resize_width, R, R)
                else:
                    d.resize_height = d.resize_width = R
                    d.out_top = d.out_left = 0
                d.flip = 0
        return descs, augs, off

    def pack(self, images: Sequence) -> Tuple[torch.Tensor, int]:
        """Copies the decoded images back to back into a (re-used) pinned host buffer."""
        total = sum(int(np.prod(im.shape)) for im in images)
        self._slot = (self._slot + 1) % len(self._ring)
        ent = self._ring[self._slot]
        if ent[1] is not None:
            ent[1].synchronize()                      # the upload that last read this buffer has completed
        if ent[0] is None or ent[0].numel() < total:
            ent[0] = torch.empty(max(total, 1), dtype=torch.uint8)
            if torch.cuda.is_available():
                ent[0] = ent[0].pin_memory()
        pinned = ent[0]
        off = 0
        for im in images:
            a = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
            if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
                raise ValueError("images must be uint8 HWC with 3 channels")
            n = a.numel()
            pinned[off:off + n].copy_(a.reshape(-1))
            off += n
        return pinned, total

    def __call__(self, images: Sequence, want_u8: bool = False):
        descs, augs, total = self.describe_aug([(int(im.shape[0]), int(im.shape[1])) for im in images])
        host, n = self.pack(images)
        src = host[:n].to(self.engine.device if hasattr(self.engine, "device") else "cuda", non_blocking=True)
        if src.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(src.device))
            self._ring[self._slot][1] = ev
        if augs is None and not self.fill_outside:
            return self.engine.preprocess(src, descs, self.size, self.mean, self.std, self.out_dtype, want_u8)
        return self.engine.preprocess_aug(src, descs, augs, self.size, self.mean, self.std, self.out_dtype, want_u8, self.fill_outside)

    def describe_encoded(self, blobs: Sequence, infos=None, decoded=None):
        """(probe results, (height, width) per file, image descriptors, augmentation descriptors or None) for JPEG files: the sizes come
        from the frame headers, and the random parameters are drawn as `__call__` draws them for decoded images of those sizes.
        infos / decoded: what `jpeg.probe` / `jpeg.shapes_of` gave for these files, when the caller has them already."""
        from . import jpeg
        infos = [jpeg.probe(b) for b in blobs] if infos is None else infos
        shapes, _ = jpeg.shapes_of(blobs, infos, decoded)
        descs, augs, _ = self.describe_aug(shapes)
        return infos, shapes, descs, augs

    def _run(self, src, descs, augs, want_u8):
        if augs is None and not self.fill_outside:
            return self.engine.preprocess(src, descs, self.size, self.mean, self.std, self.out_dtype, want_u8)
        return self.engine.preprocess_aug(src, descs, augs, self.size, self.mean, self.std, self.out_dtype, want_u8, self.fill_outside)

    def from_encoded(self, blobs: Sequence, want_u8: bool = False, check: bool = True, infos=None, decoded=None):
        """`__call__` for a list of JPEG files (bytes): they are decoded on the device (mvlpt_amd.jpeg.decode_batch; Pillow for the files
        the device does not take), and the same generator state gives the batch `__call__` gives for the Pillow-decoded arrays, bit for
        bit.  check=False leaves the decode status unread (no synchronisation; corrupt files keep the device's pixels).
        infos / decoded ({index: pixels} of host-route files): host work a loader's threads have done already."""
        from . import jpeg
        infos, _, descs, augs = self.describe_encoded(blobs, infos, decoded)
        src, _, _, _ = jpeg.decode_batch(self.engine, blobs, check=check, infos=infos, decoded=decoded)
        return self._run(src, descs, augs, want_u8)

    def from_resident(self, image_set, indices: Sequence[int], want_u8: bool = False):
        """`__call__` for images that lie decoded in a resident device buffer (mvlpt_amd.data.ResidentImageSet: `buf`, `offsets`,
        `shapes`): nothing is packed or uploaded but the descriptors, whose `offset` is the image's place in the set (64 bits), and the
        whole set is the source of the one preprocess launch.  The same generator state draws what `__call__` draws for these images."""
        indices = [int(i) for i in indices]
        descs, augs, _ = self.describe_aug([image_set.shapes[i] for i in indices])
        for d, i in zip(descs, indices):
            d.offset = int(image_set.offsets[i])
        return self._run(image_set.buf, descs, augs, want_u8)


class ViewTransform:
    """V views of every image in ONE preprocess launch (test-time prompt tuning, mvlpt_amd.tpt): [G, V, 3, size, size].
    View 0 of an image carries the descriptor of `test` (a train=False DeviceTransform: Resize + CenterCrop), views 1 .. V-1 those of
    `train` (a train=True one: random_resized_crop, random_flip and whatever INPUT.TRANSFORMS adds), drawn image after image from
    `train`'s generator: the same state draws, for image i, what `train.describe_aug([shape_i] * (V - 1))` draws.  All V descriptors
    of an image share one `offset`: the image lies in the source once (a resident set's buffer, one packed upload, or one device
    decode), never V times.  With augmentations in `train` the launch is the augmenting one and view 0 gets an empty augmentation
    descriptor (no colour operation, no grayscale, no hole)."""

    def __init__(self, test: DeviceTransform, train: DeviceTransform, n_views: int):
        if test.train or not train.train:
            raise ValueError("ViewTransform(test, train): `test` must be a train=False transform and `train` a train=True one")
        if (test.size, test.mean, test.std, test.out_dtype) != (train.size, train.mean, train.std, train.out_dtype):
            raise ValueError("the test and train transforms of a ViewTransform must share size, mean / std (keep 'normalize' in "
                             "INPUT.TRANSFORMS) and output type: the views are one launch")
        if int(n_views) < 1:
            raise ValueError(f"n_views must be at least 1, got {n_views}")
        self.test, self.train, self.n_views = test, train, int(n_views)
        self.engine, self.size = train.engine, train.size

    def describe_views(self, shapes: Sequence[Tuple[int, int]], offsets: Sequence[int]):
        """(image descriptors [G * V], augmentation descriptors [G * V] or None), image-major; `offsets` [G]: each image's place in
        the source."""
        V, G = self.n_views, len(shapes)
        descs = (_lib.MvlptImageDesc * (G * V))()
        augs = (_lib.MvlptAugmentDesc * (G * V))() if self.train.augments else None
        for g, (shape, off) in enumerate(zip(shapes, offsets)):
            d0, _, _ = self.test.describe_aug([shape])
            descs[g * V] = d0[0]
            if V > 1:
                dt, at, _ = self.train.describe_aug([shape] * (V - 1))
                for j in range(V - 1):
                    descs[g * V + 1 + j] = dt[j]
                    if augs is not None:
                        augs[g * V + 1 + j] = at[j]
            for j in range(V):
                descs[g * V + j].offset = int(off)
        return descs, augs

    def _run(self, src, descs, augs):
        tr = self.train
        if augs is None and not tr.fill_outside:
            out = self.engine.preprocess(src, descs, self.size, tr.mean, tr.std, tr.out_dtype, False)
        else:
            out = self.engine.preprocess_aug(src, descs, augs, self.size, tr.mean, tr.std, tr.out_dtype, False, tr.fill_outside)
        return out.view(len(descs) // self.n_views, self.n_views, *out.shape[1:])

    def from_resident(self, image_set, indices: Sequence[int]):
        indices = [int(i) for i in indices]
        descs, augs = self.describe_views([image_set.shapes[i] for i in indices], [image_set.offsets[i] for i in indices])
        return self._run(image_set.buf, descs, augs)

    def __call__(self, images: Sequence):
        """Decoded uint8 HWC arrays: packed and uploaded once."""
        shapes, offsets, off = [], [], 0
        for im in images:
            shapes.append((int(im.shape[0]), int(im.shape[1])))
            offsets.append(off)
            off += shapes[-1][0] * shapes[-1][1] * 3
        descs, augs = self.describe_views(shapes, offsets)
        tr = self.train
        host, n = tr.pack(images)
        src = host[:n].to(self.engine.device if hasattr(self.engine, "device") else "cuda", non_blocking=True)
        if src.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(src.device))
            tr._ring[tr._slot][1] = ev
        return self._run(src, descs, augs)

    def from_encoded(self, blobs: Sequence, check: bool = True, infos=None, decoded=None):
        """JPEG files (bytes): ONE device decode of the batch (mvlpt_amd.jpeg.decode_batch), V descriptors pointing at each image."""
        from . import jpeg
        src, offsets, shapes, _ = jpeg.decode_batch(self.engine, blobs, check=check, infos=infos, decoded=decoded)
        descs, augs = self.describe_views([tuple(s) for s in shapes], [int(o) for o in offsets])
        return self._run(src, descs, augs)


def build_view_transform(cfg, engine, n_views: int, generator: Optional[torch.Generator] = None) -> ViewTransform:
    """The ViewTransform of INPUT.*: view 0 as Dassl's test transform, the others as its train transform."""
    return ViewTransform(build_device_transform(cfg, engine, train=False), build_device_transform(cfg, engine, train=True, generator=generator),
                         n_views)


def build_device_transform(cfg, engine, train: bool = True, **kwargs) -> DeviceTransform:
    """The transform Dassl's `build_transform(cfg, is_train=train)` would build from INPUT.TRANSFORMS and its parameters (same key names
    and defaults), on the device.  Testing is Dassl's Resize(size) + CenterCrop(size) + normalize; the names are checked either way."""
    inp = cfg.INPUT
    return DeviceTransform(engine, size=int(inp.SIZE[0]), train=train, center_crop=True, transforms=check_transforms(inp.TRANSFORMS),
                           colorjitter=(inp.COLORJITTER_B, inp.COLORJITTER_C, inp.COLORJITTER_S, inp.COLORJITTER_H), rgs_p=inp.RGS_P,
                           crop_padding=inp.CROP_PADDING, cutout_n=inp.CUTOUT_N, cutout_len=inp.CUTOUT_LEN, **kwargs)
