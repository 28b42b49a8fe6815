"""The small image dataset of tests/test_data_host.py and tests/test_hip_data.py, written with Pillow: 3 classes x (6 train, 2 val, 3 test)
files of 17 x 23 .. 64 x 48 pixels in the folder layout root/{train,val,test}/<class>/, plus the CoOp split file of the same items.
Among them a 4:2:0 file with odd sizes, a grayscale JPEG, a file with a restart interval (all three decoded by the device), one
progressive JPEG and one PNG (both decoded by Pillow), in the train split; the last test file is a plain 4:4:4 JPEG."""
import json
import os

import numpy as np

CLASSES = ("heron", "otter", "badger")           # sorted by name: badger 0, heron 1, otter 2
COUNTS = {"train": 6, "val": 2, "test": 3}
SIZES = [(17, 23), (64, 48), (23, 17), (33, 47), (48, 64), (40, 40), (31, 64), (64, 19), (25, 58)]      # (height, width)
N_HOST_TRAIN = 2                                 # the progressive file and the PNG


def _pixels(rng, h, w):
    from PIL import Image
    low = rng.integers(0, 256, (3, 4, 3)).astype(np.uint8)
    a = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC)).astype(np.int16) + rng.integers(-20, 21, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def write_dataset(root, seed=0, prefix=""):
    """Writes the dataset under `root`; returns {"train" | "val" | "test": [(path, label, class name)]} in `read_folders` order
    (classes sorted, files sorted) and writes root/split.json with the same items."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    classes = sorted(CLASSES)
    items, k = {}, 0
    for split, n in COUNTS.items():
        items[split] = []
        for label, c in enumerate(classes):
            folder = os.path.join(root, split, c)
            os.makedirs(folder, exist_ok=True)
            for j in range(n):
                h, w = SIZES[k % len(SIZES)]
                k += 1
                im = Image.fromarray(_pixels(rng, h, w))
                name, kw = f"{prefix}{j}.jpg", dict(quality=85, subsampling=0)
                if split == "train" and label == 0:
                    if j == 0:
                        im, kw = Image.fromarray(_pixels(rng, 23, 17)), dict(quality=90, subsampling=2)      # 4:2:0, odd sizes
                    elif j == 1:
                        im = im.convert("L")                                                                 # grayscale JPEG
                    elif j == 2:
                        kw = dict(quality=90, subsampling=2, restart_marker_rows=1)                          # restart interval
                    elif j == 3:
                        kw = dict(quality=80, progressive=True)                                              # host route
                    elif j == 4:
                        name, kw = f"{prefix}{j}.png", None                                                   # not a JPEG
                path = os.path.join(folder, name)
                if kw is None:
                    im.save(path, "PNG")
                else:
                    im.save(path, "JPEG", **kw)
                items[split].append((path, label, c))
        items[split].sort(key=lambda t: (t[1], os.path.basename(t[0])))
    with open(os.path.join(root, "split.json"), "w") as f:
        json.dump({s: [[os.path.relpath(p, root), lab, c] for p, lab, c in rows] for s, rows in items.items()}, f)
    return items


def pillow_arrays(paths):
    from PIL import Image
    return [np.asarray(Image.open(p).convert("RGB")) for p in paths]
