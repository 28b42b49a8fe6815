"""Baseline JPEG decode on the device (csrc/jpeg.hip): compressed files -> the packed uint8 HWC RGB device buffer
`mvlpt_preprocess(_aug)` reads, bit-identical to Pillow's `Image.open(f).convert("RGB")`.

The host parses the headers (`mvlpt_jpeg_probe`) and uploads the compressed bytes -- about a fifth of the decoded pixels -- and the device
does the arithmetic.  A file the device does not take (progressive, CMYK, other sampling factors, ...: `probe(blob).route`) is decoded
by Pillow here and its pixels are uploaded into the same buffer, so a batch always comes back complete; only a file that Pillow cannot
read either raises."""
from __future__ import annotations

import ctypes as C
import io
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

ROUTE_NAMES = ("device", "malformed", "frame", "scans", "colour", "sampling", "tables", "restart", "size")


class JpegInfo(NamedTuple):
    height: int
    width: int
    components: int
    h_samp: int
    v_samp: int
    restart_interval: int
    n_segments: int
    route: int                       # _lib.JPEG_ROUTE_*: 0 = the device decodes it

    @property
    def reason(self) -> str:
        return ROUTE_NAMES[self.route]


def _bytes(blob) -> bytes:
    return blob if isinstance(blob, bytes) else bytes(blob)


def probe(blob) -> JpegInfo:
    """Headers of one file (host only, no device): size, components, sampling, restart interval, segments, and who decodes it."""
    blob = _bytes(blob)
    info = _lib.MvlptJpegInfo()
    _lib.check(_lib.lib.mvlpt_jpeg_probe(blob, len(blob), C.byref(info)), None, "jpeg_probe")
    return JpegInfo(*(int(getattr(info, n)) for n, _ in _lib.MvlptJpegInfo._fields_))


def workspace_bytes(infos: Sequence[JpegInfo]) -> int:
    arr = (_lib.MvlptJpegInfo * max(len(infos), 1))(*[_lib.MvlptJpegInfo(*i) for i in infos])
    out = C.c_int64()
    _lib.check(_lib.lib.mvlpt_jpeg_workspace_bytes(arr, len(infos), C.byref(out)), None, "jpeg_workspace_bytes")
    return int(out.value)


def pillow_rgb(blob) -> np.ndarray:
    """The host route: uint8 [H, W, 3] as Pillow decodes the file."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(_bytes(blob))).convert("RGB"))


def header_has_size(f: JpegInfo) -> bool:
    """the frame header of the probed file gives its size (else only decoding it does: no JPEG, or malformed)"""
    return f.height > 0 and f.width > 0 and f.route not in (_lib.JPEG_ROUTE_MALFORMED, _lib.JPEG_ROUTE_SIZE)


def shapes_of(blobs: Sequence, infos: Optional[Sequence[JpegInfo]] = None, decoded: Optional[dict] = None) -> Tuple[List[Tuple[int, int]], dict]:
    """((height, width) per file, {index: pixels} of the files that had to be decoded to learn it).  The frame header gives the size
    of every file that has one; a file without is decoded by Pillow, unless `decoded` holds its pixels already."""
    infos = [probe(b) for b in blobs] if infos is None else infos
    shapes, decoded = [], {} if decoded is None else dict(decoded)
    for k, (blob, f) in enumerate(zip(blobs, infos)):
        if header_has_size(f):
            shapes.append((f.height, f.width))
        else:
            if k not in decoded:
                decoded[k] = pillow_rgb(blob)
            shapes.append(tuple(decoded[k].shape[:2]))
    return shapes, decoded


class _PinnedRing:
    """Three pinned staging buffers, each guarded by the event of the last copy that read it (as DeviceTransform.pack)."""

    def __init__(self):
        self._ring = [[None, None] for _ in range(3)]
        self._slot = -1

    def take(self, nbytes: int) -> torch.Tensor:
        self._slot = (self._slot + 1) % len(self._ring)
        ent = self._ring[self._slot]
        if ent[1] is not None:
            ent[1].synchronize()
        if ent[0] is None or ent[0].numel() < nbytes:
            ent[0] = torch.empty(max(nbytes, 1), dtype=torch.uint8)
            if torch.cuda.is_available():
                ent[0] = ent[0].pin_memory()
        return ent[0]

    def guard(self, device):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._ring[self._slot][1] = ev


def _rings(engine):
    r = getattr(engine, "_jpeg_rings", None)
    if r is None:
        r = engine._jpeg_rings = (_PinnedRing(), _PinnedRing())        # compressed bytes, fallback pixels
    return r


_UPLOAD_BLOCK = 64 << 20          # pixels go up through pinned blocks of about this size (one image may exceed it)


def _upload_pixels(ring: _PinnedRing, dst: torch.Tensor, items: Sequence[Tuple[int, np.ndarray]]):
    """pixels of (offset, uint8 [H, W, 3]) pairs into dst, through pinned blocks of about _UPLOAD_BLOCK bytes"""
    items = list(items)
    lo = 0
    while lo < len(items):
        hi, total = lo, 0
        while hi < len(items) and (hi == lo or total + items[hi][1].size <= _UPLOAD_BLOCK):
            total += items[hi][1].size
            hi += 1
        host = ring.take(total)
        host_np = host.numpy()
        at = 0
        for off, a in items[lo:hi]:
            host_np[at:at + a.size] = a.reshape(-1)
            dst[off:off + a.size].copy_(host[at:at + a.size], non_blocking=True)
            at += a.size
        ring.guard(dst.device)
        lo = hi


def upload_pixels(engine, dst: torch.Tensor, items: Sequence[Tuple[int, np.ndarray]]):
    """host-decoded images, (offset, uint8 [H, W, 3]) pairs, into the device buffer dst through the engine's pinned pixel ring"""
    _upload_pixels(_rings(engine)[1], dst, items)


def decode_batch(engine, blobs: Sequence, check: bool = True, infos: Optional[Sequence[JpegInfo]] = None, decoded: Optional[dict] = None):
    """Decodes a list of JPEG files (bytes).  Returns (buf, offsets, shapes, status):
      buf      uint8 device tensor, the images back to back as [H, W, 3] -- the layout MvlptImageDesc.offset describes
      offsets  byte offset of each image in buf;  shapes: (height, width) of each
      status   int32 device tensor [B]: 0 decoded on the device, -1 decoded by Pillow (route != device), > 0 corrupt entropy data
    check=True reads the 4 * B status bytes back (one synchronisation) and decodes the flagged files again with Pillow, replacing their
    pixels where Pillow can read them; check=False returns the status unread, so a training loop need not synchronise.
    `decoded` ({index: pixels}) hands in host-route files somebody decoded already (a loader's worker threads)."""
    device = engine.device
    blobs = [_bytes(b) for b in blobs]
    infos = [probe(b) for b in blobs] if infos is None else list(infos)
    shapes, dec = shapes_of(blobs, infos, decoded)
    offsets, total = [], 0
    for h, w in shapes:
        offsets.append(total)
        total += h * w * 3
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=device)[:total]
    status, _ = decode_into(engine, blobs, buf, offsets, shapes, infos, dec, check)
    return buf, offsets, shapes, status


def decode_into(engine, blobs: Sequence, dst: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Tuple[int, int]],
                infos: Sequence[JpegInfo], decoded: Optional[dict] = None, check: bool = True):
    """`decode_batch` into a buffer the caller owns: file k goes to dst[offsets[k] : offsets[k] + h * w * 3], wherever that lies in dst
    (64-bit offsets; a resident image set is filled this way, super-batch by super-batch, with no copy of device-decoded pixels).
    shapes / infos are those of `shapes_of` / `probe`; decoded = {index: pixels} of host-route files that are decoded already.
    Returns (status, status_host): the int32 device tensor of `decode_batch` and, with check=True, its host copy (else None)."""
    device = engine.device
    blobs = [_bytes(b) for b in blobs]
    B = len(blobs)
    decoded = {} if decoded is None else decoded
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B == 0:
        return status, (np.zeros(0, np.int32) if check else None)
    if dst.dtype != torch.uint8 or not dst.is_contiguous() or not dst.is_cuda:
        raise ValueError("dst must be a contiguous uint8 device tensor")
    for k, ((h, w), off) in enumerate(zip(shapes, offsets)):
        if off < 0 or off + h * w * 3 > dst.numel():
            raise ValueError(f"image {k} ({h} x {w}) does not fit dst at offset {off}")
    comp_ring, pix_ring = _rings(engine)
    sizes = [len(b) for b in blobs]
    src_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    n = int(sum(sizes))
    host = comp_ring.take(n)
    host_np = host.numpy()
    for o, b in zip(src_off, blobs):
        host_np[o:o + len(b)] = np.frombuffer(b, np.uint8)
    status_host = None
    with torch.cuda.device(device):
        src = host[:n].to(device, non_blocking=True)
        comp_ring.guard(device)
        i64 = C.c_int64 * B
        _lib.check(_lib.lib.mvlpt_jpeg_decode(engine.h, C.c_void_p(host.data_ptr()), C.c_void_p(src.data_ptr()), i64(*[int(v) for v in src_off]),
                                              i64(*sizes), B, C.c_void_p(dst.data_ptr()), dst.numel(), i64(*[int(v) for v in offsets]),
                                              C.c_void_p(status.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   engine.h, "jpeg_decode")
        host_route = []
        for k, f in enumerate(infos):
            if f.route != _lib.JPEG_ROUTE_DEVICE:
                a = decoded[k] if k in decoded else pillow_rgb(blobs[k])
                if tuple(a.shape[:2]) != tuple(shapes[k]):
                    raise ValueError(f"image {k}: Pillow decodes {a.shape[:2]}, the frame header says {shapes[k]}")
                host_route.append((offsets[k], a))
        if host_route:
            _upload_pixels(pix_ring, dst, host_route)
        if check:
            status_host = status.cpu().numpy()
            again = []
            for k in np.flatnonzero(status_host > 0):
                try:
                    a = pillow_rgb(blobs[k])
                except Exception:                                    # Pillow cannot read it either: the device's pixels stand
                    continue
                if tuple(a.shape[:2]) == tuple(shapes[k]):
                    again.append((offsets[k], a))
            if again:
                _upload_pixels(pix_ring, dst, again)
    return status, status_host
