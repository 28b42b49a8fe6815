"""Image files -> training and evaluation batches through the device input pipeline: the data manager every trainer
builds when `DATASET.SOURCES` names datasets, in place of Dassl's `DataManager` + torch `DataLoader` (trainers/mvlpt.py:585-735).

Few-shot prompt tuning trains many epochs over the same few thousand files, so a split is decoded ONCE (`mvlpt_jpeg_decode`, Pillow for
the files the device does not take) into one uint8 device buffer, a `ResidentImageSet`; a step's input is then a descriptor table into
that buffer and one `mvlpt_preprocess(_aug)` launch (`DeviceTransform.from_resident`).  A split that does not fit
`DATALOADER.RESIDENT_BYTES` streams instead: host threads read (and probe) the files of the next batches while a step runs, and
`DeviceTransform.from_encoded` decodes and transforms them.  Either way the batches are, bit for bit, what `DeviceTransform.__call__`
gives for the Pillow-decoded files in the same order: the loader adds no arithmetic.

Threads do host work only (file reads, `jpeg.probe`, Pillow decodes); every engine call is made by the consuming thread, in program
order, on the stream the engine already uses: its grow-only workspaces have one caller.

The record type, the CoOp split file and the class subsampling follow the reference's readers (datasets/oxford_pets.py:100-186); there
is one generic reader per layout here, no per-dataset module."""
from __future__ import annotations

import json
import math
import os
import random
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, jpeg
from .transforms import build_device_transform, build_view_transform

SUPER_BATCH = 1024                   # files per mvlpt_jpeg_decode call while a resident set is filled
MAX_WORKERS = 16


class Datum(NamedTuple):
    impath: str
    label: int
    domain: int = 0
    classname: str = ""


# ------------------------------------------------------------------------------------------------ readers (host only)
def read_split_json(path: str, image_dir: str) -> Tuple[List[Datum], List[Datum], List[Datum]]:
    """(train, val, test) of a CoOp split file: {"train": [[relative path, label, class name], ...], "val": ..., "test": ...}; the
    paths are relative to `image_dir`."""
    with open(path) as f:
        split = json.load(f)

    def convert(rows):
        return [Datum(os.path.join(image_dir, rel), int(label), 0, str(cname)) for rel, label, cname in rows]
    return convert(split["train"]), convert(split.get("val", [])), convert(split["test"])


def read_folders(root: str) -> Tuple[List[Datum], List[Datum], List[Datum]]:
    """(train, val, test) of the layout root/{train,val,test}/<class name>/<file>: the classes are the folders of `train`, sorted by
    name, and the label is the position in that order; files are taken in sorted order; `val` may be missing (an empty list)."""
    train_dir = os.path.join(root, "train")
    classes = sorted(d for d in os.listdir(train_dir) if os.path.isdir(os.path.join(train_dir, d)))
    label_of = {c: k for k, c in enumerate(classes)}

    def read(split, optional=False):
        base = os.path.join(root, split)
        if not os.path.isdir(base):
            if optional:
                return []
            raise FileNotFoundError(f"{base}: no such folder")
        items = []
        for c in sorted(d for d in os.listdir(base) if os.path.isdir(os.path.join(base, d))):
            if c not in label_of:
                raise ValueError(f"{base}/{c}: a class that {train_dir} does not have")
            folder = os.path.join(base, c)
            for name in sorted(os.listdir(folder)):
                if os.path.isfile(os.path.join(folder, name)):
                    items.append(Datum(os.path.join(folder, name), label_of[c], 0, c))
        return items
    return read("train"), read("val", optional=True), read("test")


def few_shot(items: Sequence[Datum], num_shots: int, rng: random.Random) -> List[Datum]:
    """Per label, taken in ascending order, `num_shots` items drawn without replacement (`rng.sample`); a label with fewer items keeps
    all of them, in their order; num_shots < 1 keeps everything.
    This restates Dassl's `generate_fewshot_dataset`.  Dassl is not installed where this is built, so the sampling is RESTATED AND NOT
    PINNED against it: the same seed need not pick the files Dassl picks."""
    if num_shots < 1:
        return list(items)
    by_label: Dict[int, List[Datum]] = defaultdict(list)
    for it in items:
        by_label[it.label].append(it)
    out: List[Datum] = []
    for label in sorted(by_label):
        group = by_label[label]
        out.extend(rng.sample(group, num_shots) if len(group) >= num_shots else group)
    return out


def subsample_classes(train: Sequence[Datum], val: Sequence[Datum], test: Sequence[Datum], subsample: str = "all"):
    """"base": the first ceil(n / 2) of the n labels `train` has, "new": the rest, each relabelled from 0; "all": as they are."""
    if subsample not in ("all", "base", "new"):
        raise ValueError(f"DATASET.SUBSAMPLE_CLASSES must be all, base or new, not {subsample!r}")
    if subsample == "all":
        return list(train), list(val), list(test)
    labels = sorted({it.label for it in train})
    m = math.ceil(len(labels) / 2)
    selected = labels[:m] if subsample == "base" else labels[m:]
    relabel = {y: k for k, y in enumerate(selected)}
    return tuple([it._replace(label=relabel[it.label]) for it in items if it.label in relabel] for items in (train, val, test))


def rank_seed(seed: int, rank: int = 0) -> int:
    """the generator seed of `rank`: `seed` itself on rank 0, apart by 1 000 003 per rank (torch's CPU generator reads 32 bits of a seed,
    so the rank cannot ride above them)"""
    return int(seed) + 1000003 * int(rank)


def _read_file(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _probe_file(path: str):
    """(probe result, (height, width)) of one file; a file whose header does not give the size is decoded by Pillow for it"""
    blob = _read_file(path)
    info = jpeg.probe(blob)
    return info, ((info.height, info.width) if jpeg.header_has_size(info) else tuple(jpeg.pillow_rgb(blob).shape[:2]))


def _read_for_device(path: str):
    """(bytes, probe result, Pillow's pixels when the device does not take the file, else None)"""
    blob = _read_file(path)
    info = jpeg.probe(blob)
    return blob, info, (None if info.route == _lib.JPEG_ROUTE_DEVICE else jpeg.pillow_rgb(blob))


def _read_for_host(path: str) -> np.ndarray:
    return jpeg.pillow_rgb(_read_file(path))


def _map(pool: Optional[ThreadPoolExecutor], fn, paths):
    return [fn(p) for p in paths] if pool is None else list(pool.map(fn, paths))


# ------------------------------------------------------------------------------------------------ resident set
class ResidentImageSet:
    """The files of `paths`, decoded, back to back as uint8 [H, W, 3] in ONE device allocation of sum(h * w * 3) bytes: `buf`, with
    `offsets[i]` / `shapes[i]` of image i.  `shapes` come from the headers (`probe_files`) before anything is decoded.  The set is filled
    in super-batches of at most SUPER_BATCH files by `jpeg.decode_into`, straight to each image's offset; files the device does not
    take (progressive or CMYK JPEGs, PNG, ...) get Pillow's pixels there.  decode="host": Pillow for every file.  The status words are
    read once per super-batch (the only synchronisations) and flagged files are decoded again by Pillow, as `decode_batch(check=True)`.
    n_device / n_host / n_corrupt: files decoded by the device / by Pillow because of their route / flagged corrupt by the device."""

    def __init__(self, engine, paths: Sequence[str], shapes: Sequence[Tuple[int, int]], decode: str = "device", workers: int = 0):
        if decode not in ("device", "host"):
            raise ValueError(f"DATALOADER.DECODE must be device or host, not {decode!r}")
        self.paths, self.shapes = list(paths), [tuple(s) for s in shapes]
        self.offsets, total = [], 0
        for h, w in self.shapes:
            self.offsets.append(total)
            total += h * w * 3
        self.resident_bytes = total
        self.n_device = self.n_host = self.n_corrupt = 0
        self.buf = torch.empty(max(total, 1), dtype=torch.uint8, device=engine.device)[:total]
        pool = ThreadPoolExecutor(max_workers=workers) if workers > 0 else None
        try:
            for lo in range(0, len(self.paths), SUPER_BATCH):
                self._fill(engine, lo, min(lo + SUPER_BATCH, len(self.paths)), decode, pool)
        finally:
            if pool is not None:
                pool.shutdown(wait=True)

    def _fill(self, engine, lo, hi, decode, pool):
        offsets, shapes = self.offsets[lo:hi], self.shapes[lo:hi]
        if decode == "host":
            arrays = _map(pool, _read_for_host, self.paths[lo:hi])
            for k, a in enumerate(arrays):
                if tuple(a.shape[:2]) != shapes[k]:
                    raise ValueError(f"{self.paths[lo + k]}: Pillow decodes {a.shape[:2]}, the header says {shapes[k]}")
            jpeg.upload_pixels(engine, self.buf, list(zip(offsets, arrays)))
            self.n_host += hi - lo
            return
        got = _map(pool, _read_for_device, self.paths[lo:hi])
        blobs, infos = [g[0] for g in got], [g[1] for g in got]
        decoded = {k: g[2] for k, g in enumerate(got) if g[2] is not None}
        _, status = jpeg.decode_into(engine, blobs, self.buf, offsets, shapes, infos, decoded, check=True)
        self.n_host += int((status < 0).sum())
        self.n_corrupt += int((status > 0).sum())
        self.n_device += int((status == 0).sum())

    def __len__(self):
        return len(self.paths)


def probe_files(paths: Sequence[str], workers: int = 0) -> List[Tuple[int, int]]:
    """(height, width) of every file, from its header where it has one (host only; `workers` threads)"""
    pool = ThreadPoolExecutor(max_workers=workers) if workers > 0 else None
    try:
        return [s for _, s in _map(pool, _probe_file, paths)]
    finally:
        if pool is not None:
            pool.shutdown(wait=True)


# ------------------------------------------------------------------------------------------------ loader
class DeviceLoader:
    """Iterable over the batches of `items` (a list of Datum): {"img": device [B, 3, R, R], "label": device int64 [B], "domain": int64 [B]
    (host, the trainers read it there), "impath": list}.  `dataset` is the list, `batch_size` and `len()` as a torch DataLoader's.
    train=True : a fresh permutation per epoch from torch.Generator().manual_seed(rank_seed(SEED + epoch, rank)), where `epoch` counts
                 this loader's `__iter__` calls; drop_last; the transform of INPUT.TRANSFORMS with its parameters drawn from ONE
                 generator seeded rank_seed(SEED, rank) when the loader is bound, batch after batch.
    train=False: every item once, in order, the last batch partial; Resize + CenterCrop + normalize.
    The loader is born unbound (the engine exists only after build_model); `bind(engine, image_set)` makes it iterable: with a
    ResidentImageSet of its files it takes the resident route, without one it streams."""

    def __init__(self, cfg, items: Sequence[Datum], train: bool, rank: int = 0):
        self.cfg, self.dataset, self.train, self.rank = cfg, list(items), train, rank
        self.batch_size = int(cfg.DATALOADER.TRAIN_X.BATCH_SIZE if train else cfg.DATALOADER.TEST.BATCH_SIZE)
        self.drop_last = train
        self.decode = cfg.DATALOADER.DECODE
        self.workers = max(0, min(int(cfg.DATALOADER.NUM_WORKERS), MAX_WORKERS))
        self.epoch = 0
        self.engine = self.transform = self.image_set = None
        self.n_views = 0          # > 0 (request_views): "img" is [B, n_views, 3, R, R], view 0 the test view (test-time prompt tuning)
        self._labels = torch.tensor([it.label for it in self.dataset], dtype=torch.int64)
        self._domains = torch.tensor([it.domain for it in self.dataset], dtype=torch.int64)
        self._pools: List[ThreadPoolExecutor] = []

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def bind(self, engine, image_set: Optional[ResidentImageSet] = None):
        self.engine, self.image_set = engine, image_set
        if self.n_views > 0:
            gen = torch.Generator().manual_seed(rank_seed(self.cfg.SEED, self.rank))
            self.transform = build_view_transform(self.cfg, engine, self.n_views, generator=gen)
            return
        gen = torch.Generator().manual_seed(rank_seed(self.cfg.SEED, self.rank)) if self.train else None
        self.transform = build_device_transform(self.cfg, engine, train=self.train, generator=gen)

    def request_views(self, n_views: int) -> None:
        """Serve `n_views` views per image from now on (mvlpt_amd.transforms.ViewTransform; 0: the plain batches again).  Evaluation
        loaders only; a bound loader rebuilds its transform, with a freshly seeded generator."""
        if self.train:
            raise ValueError("views are served by the evaluation loaders (test-time prompt tuning), not by the train loader")
        self.n_views = int(n_views)
        if self.engine is not None:
            self.bind(self.engine, self.image_set)

    def order(self, epoch: int) -> List[int]:
        """the item indices of `epoch`, in the order they are served"""
        n = len(self.dataset)
        if not self.train:
            return list(range(n))
        g = torch.Generator().manual_seed(rank_seed(self.cfg.SEED + epoch, self.rank))
        return torch.randperm(n, generator=g).tolist()

    def _index_batches(self, epoch):
        order, B = self.order(epoch), self.batch_size
        return [order[k * B:(k + 1) * B] for k in range(len(self))]

    def _batch(self, idx, img):
        dev = img.device
        return {"img": img, "label": self._labels[idx].to(dev), "domain": self._domains[idx], "impath": [self.dataset[i].impath for i in idx]}

    def __iter__(self):
        if self.transform is None:
            raise RuntimeError("this loader is not bound to an engine yet: the data manager's bind(engine) runs at the end of the "
                               "trainer's build_model; call dm.bind(engine) before iterating it elsewhere")
        if self.train and len(self) == 0:
            raise ValueError(f"the train set has {len(self.dataset)} images, fewer than one batch of {self.batch_size} (drop_last)")
        epoch, self.epoch = self.epoch, self.epoch + 1
        batches = self._index_batches(epoch)
        return self._resident(batches) if self.image_set is not None else self._stream(batches)

    def ordered(self):
        """Every item once, in dataset order, the last batch partial, through THIS loader's transform: a train loader's augmentation
        parameters go on from its generator, so every pass draws them afresh.  The pass a feature cache is built from (Tip-Adapter's
        build_cache_model reads its few-shot set with shuffle=False under the train transform).  It is not an epoch: `epoch` and the
        permutations of `__iter__` stay where they are.  len(self.ordered_batches()) batches."""
        if self.transform is None:
            raise RuntimeError("this loader is not bound to an engine yet: call dm.bind(engine) before iterating it")
        batches = self.ordered_batches()
        return self._resident(batches) if self.image_set is not None else self._stream(batches)

    def ordered_batches(self) -> List[List[int]]:
        n, B = len(self.dataset), self.batch_size
        return [list(range(k, min(k + B, n))) for k in range(0, n, B)]

    def _resident(self, batches):
        for idx in batches:
            yield self._batch(idx, self.transform.from_resident(self.image_set, idx))

    def _stream(self, batches):
        """Host threads read the files of the next two batches (and probe them, or decode them with Pillow where that is the route)
        while the consumer works; the decode, the uploads and the transform are enqueued here, by the consumer."""
        read = _read_for_host if self.decode == "host" else _read_for_device
        paths = [[self.dataset[i].impath for i in idx] for idx in batches]
        pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 0 else None
        if pool is not None:
            self._pools.append(pool)
        ahead = 2
        pending = []                      # per submitted batch: its list of futures
        try:
            for k, idx in enumerate(batches):
                if pool is None:
                    got = [read(p) for p in paths[k]]
                else:
                    while len(pending) < min(ahead + 1, len(batches) - k):
                        pending.append([pool.submit(read, p) for p in paths[k + len(pending)]])
                    got = [f.result() for f in pending.pop(0)]
                if self.decode == "host":
                    img = self.transform(got)
                else:
                    decoded = {j: g[2] for j, g in enumerate(got) if g[2] is not None}
                    # check=False: enqueue only, no status read per step (a corrupt file keeps the device's pixels)
                    img = self.transform.from_encoded([g[0] for g in got], check=False, infos=[g[1] for g in got], decoded=decoded)
                yield self._batch(idx, img)
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)
                if pool in self._pools:
                    self._pools.remove(pool)

    def close(self):
        """joins the reader threads of iterators that were left unfinished (the trainers call it where an epoch's loop ends)"""
        while self._pools:
            self._pools.pop().shutdown(wait=True, cancel_futures=True)


# ------------------------------------------------------------------------------------------------ data manager
class DeviceDataManager:
    """The data manager of `cfg.DATASET.SOURCES`, a list of [task name, split file or "", image folder]: with a split file the source is
    `read_split_json(split file, image folder)`, without one `read_folders(image folder)`.  Per source, in order: few-shot draws
    (DATASET.NUM_SHOTS for train, min(NUM_SHOTS, 4) for val, one random.Random(SEED) for all of them), DATASET.SUBSAMPLE_CLASSES, then
    -- as MVLPTCOOPDataManager (trainers/mvlpt.py:585-645) -- labels shifted by the class count of the sources before it and `domain`
    set to the source's index.  Attribute surface of SyntheticDataManager / MultitaskBook.
    `bind(engine)` probes the files, makes train, val and test resident in that order while DATALOADER.RESIDENT_BYTES lasts (a split
    that does not fit streams) and binds the loaders."""

    def __init__(self, cfg, rank: int = 0):
        sources = [list(s) for s in cfg.DATASET.SOURCES]
        if not sources:
            raise ValueError("DATASET.SOURCES is empty: give [task name, split file or \"\", image folder] per dataset")
        self.cfg, self.rank = cfg, rank
        rng = random.Random(cfg.SEED)
        shots = int(cfg.DATASET.NUM_SHOTS)
        self.train_x, self.val, self.test = [], [], []
        self.classnames, self.lab2cname, self.num_classes_list = [], {}, []
        self._task_names, self._id2task, self._task_class_idx, self._labelmap = [], {}, {}, {}
        offset = 0
        for domain, src in enumerate(sources):
            if len(src) != 3:
                raise ValueError(f"DATASET.SOURCES[{domain}] must be [task name, split file or \"\", image folder], got {src}")
            task, split_file, folder = src
            if task in self._labelmap:
                raise ValueError(f"DATASET.SOURCES names the task {task!r} twice")
            train, val, test = read_split_json(split_file, folder) if split_file else read_folders(folder)
            train = few_shot(train, shots, rng)
            val = few_shot(val, min(shots, 4), rng)
            train, val, test = subsample_classes(train, val, test, cfg.DATASET.SUBSAMPLE_CLASSES)
            names: Dict[int, str] = {}
            for it in list(train) + list(val) + list(test):
                if names.setdefault(it.label, it.classname) != it.classname:
                    raise ValueError(f"{task}: label {it.label} is both {names[it.label]!r} and {it.classname!r}")
            n = max(names) + 1 if names else 0
            if sorted(names) != list(range(n)) or {it.label for it in train} != set(names):
                raise ValueError(f"{task}: the labels of the train split must be 0 .. n - 1 and cover those of val and test")
            shift = lambda items: [it._replace(label=it.label + offset, domain=domain) for it in items]   # noqa: E731
            self.train_x += shift(train)
            self.val += shift(val)
            self.test += shift(test)
            cnames = [names[k] for k in range(n)]
            self.classnames += cnames
            self.lab2cname.update({offset + k: c for k, c in enumerate(cnames)})
            self.num_classes_list.append(n)
            self._task_names.append(task)
            self._id2task[domain] = task
            self._task_class_idx[task] = (offset, offset + n)
            self._labelmap[task] = cnames
            offset += n
        self.num_classes = self._num_classes = offset
        self.dataset = self
        self.num_source_domains = 1
        self.train_loader_x = DeviceLoader(cfg, self.train_x, train=True, rank=rank)
        self.train_loader_u = None
        self.val_loader = DeviceLoader(cfg, self.val, train=False, rank=rank) if self.val else None
        self.test_loader = DeviceLoader(cfg, self.test, train=False, rank=rank)
        self.image_sets: Dict[str, Optional[ResidentImageSet]] = {}
        self.engine = None

    def bind(self, engine):
        if self.engine is engine:
            return
        self.engine = engine
        cfg = self.cfg
        budget = int(cfg.DATALOADER.RESIDENT_BYTES)
        workers = max(0, min(int(cfg.DATALOADER.NUM_WORKERS), MAX_WORKERS))
        for name, loader in (("train", self.train_loader_x), ("val", self.val_loader), ("test", self.test_loader)):
            if loader is None:
                continue
            image_set = None
            if budget > 0:
                paths = [it.impath for it in loader.dataset]
                shapes = probe_files(paths, workers)
                need = sum(h * w * 3 for h, w in shapes)
                if need <= budget:
                    image_set = ResidentImageSet(engine, paths, shapes, cfg.DATALOADER.DECODE, workers)
                    budget -= need
            self.image_sets[name] = image_set
            loader.bind(engine, image_set)

    def request_views(self, n_views: int) -> None:
        """The val and test loaders serve `n_views` views per image (DeviceLoader.request_views); the train loader is untouched."""
        for loader in (self.val_loader, self.test_loader):
            if loader is not None:
                loader.request_views(n_views)

    @property
    def resident_bytes(self) -> int:
        return sum(s.resident_bytes for s in self.image_sets.values() if s is not None)
