"""Thin torch-facing wrapper over the C ABI: device pointers + the current HIP stream in, tensors out.

PyTorch is plumbing here (device memory, streams); all compute is in libmvlpt_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import DT_BF16, DT_F16, DT_F32, lib
from .weights import ClipArch, arch_from_state_dict, is_resnet

_TORCH2DT = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
_DT2TORCH = {DT_F16: torch.float16, DT_BF16: torch.bfloat16, DT_F32: torch.float32}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_device(fn):
    """Run an Engine method with the engine's GPU current: `_stream()` then returns THAT device's current stream and the
    library's internal hipMalloc / kernel launches land on it (one process per GPU, but rank r's GPU is cuda:r, not 0)."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        if torch.cuda.current_device() == self.device.index:
            return fn(self, *a, **k)
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapped


_PARTITION_STREAMS: Dict[Tuple[int, int, int], "torch.cuda.ExternalStream"] = {}


def partition_stream(device: torch.device, cu_first: int, cu_count: int) -> "torch.cuda.Stream":
    """A torch view of a stream that owns logical compute units [cu_first, cu_first + cu_count) of `device`
    (mvlpt_stream_create_cus, include/mvlpt_hip.h).  One stream per (device, range), kept for the life of the process."""
    key = (device.index, cu_first, cu_count)
    st = _PARTITION_STREAMS.get(key)
    if st is None:
        h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(lib.mvlpt_stream_create_cus(cu_first, cu_count, C.byref(h)), None, "stream_create_cus")
        st = _PARTITION_STREAMS[key] = torch.cuda.ExternalStream(h.value, device=device)
    return st


def device_cus(device: torch.device) -> int:
    with torch.cuda.device(device):
        return int(lib.mvlpt_stream_cus(None))


def set_stream_cu_cap(stream: "torch.cuda.Stream", n: int) -> None:
    """Grid cap of `stream` (mvlpt_stream_set_cu_cap): persistent / grid-stride launches enqueued on it from now on occupy at most
    n (rounded down to a multiple of 8) compute units; n <= 0 clears it.  Host state: no synchronisation."""
    _lib.check(lib.mvlpt_stream_set_cu_cap(C.c_void_p(stream.cuda_stream), int(n)), None, "stream_set_cu_cap")


def stream_cus(stream: Optional["torch.cuda.Stream"] = None) -> int:
    """Compute units the launchers size the grids of `stream` (default: the current one) by (mvlpt_stream_cus)."""
    return int(lib.mvlpt_stream_cus(C.c_void_p(stream.cuda_stream) if stream is not None else _stream()))


def _host_ranges(class_lo, class_hi, G: int, n_cls: int):
    """Host class ranges -> (int32 ctypes arrays lo, hi, S).  Checked here as well as in the library; never touches the device."""
    if any(isinstance(t, torch.Tensor) and t.is_cuda for t in (class_lo, class_hi)):
        raise ValueError("class ranges are host arrays (a device tensor would have to be read back)")
    lo = [int(v) for v in (class_lo.tolist() if hasattr(class_lo, "tolist") else class_lo)]
    hi = [int(v) for v in (class_hi.tolist() if hasattr(class_hi, "tolist") else class_hi)]
    if len(lo) != G or len(hi) != G:
        raise ValueError(f"class ranges must have one entry per group ({G}), got {len(lo)} / {len(hi)}")
    if any(not (0 <= a <= b <= n_cls) for a, b in zip(lo, hi)):
        raise ValueError(f"class ranges must satisfy 0 <= lo <= hi <= {n_cls}")
    S = sum(b - a for a, b in zip(lo, hi))
    if S == 0:
        raise ValueError("every class range is empty")
    return (C.c_int32 * G)(*lo), (C.c_int32 * G)(*hi), S


def _req(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor: mvlpt_amd has no CPU path")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


class _TxtState(NamedTuple):
    """What text_bwd / text_bwd_deep need of the last saving text forward; the tensors stay alive for the library's backward.
    deep: text_fwd_deep made the record, with or without deep prompts."""
    ctx_shape: Optional[Tuple[int, ...]]
    layout: torch.Tensor
    eot: torch.Tensor
    ctx_deep: Optional[torch.Tensor]
    deep: bool


_ACTIVATIONS = {"quick_gelu": _lib.ACT_QUICKGELU, "gelu": _lib.ACT_GELU}      # MODEL.BACKBONE.ACTIVATION -> MVLPT_ACT_*


class Engine:
    """One handle per process per GPU (include/mvlpt_hip.h)."""

    def __init__(self, arch: ClipArch, compute_dtype: str = "fp16", device: Optional[torch.device] = None,
                 activation: str = "quick_gelu"):
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation = {activation!r}: the accepted values are 'quick_gelu' and 'gelu'")
        if not torch.cuda.is_available():
            raise RuntimeError("mvlpt_amd.Engine needs a HIP device (no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.index is None:
            self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.arch = arch
        self.dt = {"fp16": DT_F16, "bf16": DT_BF16}[compute_dtype]
        self.torch_dtype = _DT2TORCH[self.dt]
        self.resnet = is_resnet(arch)
        h = C.c_void_p()
        if self.resnet:
            # the image tower is CLIP's ModifiedResNet: frozen, forward-only, fp16 (include/mvlpt_hip.h: mvlpt_create_resnet)
            if compute_dtype != "fp16":
                raise ValueError("a ResNet backbone computes in fp16 only (compute_dtype='bf16' is not supported)")
            a = _lib.MvlptArch(0, 0, 0, 0, 0, arch.context_length, arch.transformer_width, arch.transformer_layers,
                               arch.transformer_heads, arch.embed_dim, self.dt)
            rn = _lib.MvlptResNetArch(arch.image_resolution, arch.vision_width, (C.c_int * 4)(*arch.vision_layers),
                                      arch.vision_heads, arch.embed_dim)
            with torch.cuda.device(self.device):
                _lib.check(lib.mvlpt_create_resnet(C.byref(a), C.byref(rn), C.byref(h)), None, "mvlpt_create_resnet")
        else:
            a = _lib.MvlptArch(arch.image_resolution, arch.vision_patch_size, arch.vision_width, arch.vision_layers,
                               arch.vision_heads, arch.context_length, arch.transformer_width, arch.transformer_layers,
                               arch.transformer_heads, arch.embed_dim, self.dt)
            with torch.cuda.device(self.device):
                _lib.check(lib.mvlpt_create(C.byref(a), C.byref(h)), None, "mvlpt_create")
        self.h = h
        self.precision = _lib.PREC_SPLIT_GRAD
        self.activation = "quick_gelu"
        if activation != "quick_gelu":
            self.set_activation(activation)
        self._keep: List[torch.Tensor] = []     # tensors the library reads asynchronously / later
        self._img_state = None
        self._img_pending = None      # image_fwd_begin .. image_fwd_resume: (image, vpt, vpt_deep, masks, state for image_bwd)
        self._txt_state = None
        self._head_state = None
        self.token_table_loader = None   # weakref.WeakMethod of FrozenCLIP's "upload the token table once" (nearest_tokens: first use)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "h", None):
            lib.mvlpt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_precision(self, mode) -> None:
        """"fast" | "split_grad" (default) | "split_all" — see MVLPT_PREC_* in include/mvlpt_hip.h."""
        code = {"fast": _lib.PREC_FAST, "split_grad": _lib.PREC_SPLIT_GRAD, "split_all": _lib.PREC_SPLIT_ALL}.get(mode, mode)
        _lib.check(lib.mvlpt_set_precision(self.h, int(code)), self.h, "set_precision")
        self.precision = int(code)

    def set_activation(self, activation: str) -> None:
        """"quick_gelu" (default) | "gelu": the MLP activation of both towers (include/mvlpt_hip.h: mvlpt_set_activation).  Legal before
        a forward and after a completed step; between a saving forward and its backward the library refuses (RuntimeError)."""
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation = {activation!r}: the accepted values are 'quick_gelu' and 'gelu'")
        _lib.check(lib.mvlpt_set_activation(self.h, _ACTIVATIONS[activation]), self.h, "set_activation")
        self.activation = activation

    def get_activation(self) -> str:
        code = C.c_int(-1)
        _lib.check(lib.mvlpt_get_activation(self.h, C.byref(code)), self.h, "get_activation")
        return {v: k for k, v in _ACTIVATIONS.items()}[code.value]

    def set_text_act_ckpt(self, segments: int) -> None:
        """TRAINER.ACT_CKPT (include/mvlpt_hip.h: mvlpt_set_text_act_ckpt): the text tower keeps only the inputs of `segments`
        segments (torch's checkpoint_sequential rule) and runs all but the last one again inside text_bwd.  1: everything is
        saved.  Applies from the next text forward and to text_workspace_bytes."""
        _lib.check(lib.mvlpt_set_text_act_ckpt(self.h, int(segments)), self.h, "set_text_act_ckpt")

    def set_text_grad_len(self, grad_len: int, max_eot: int) -> None:
        """Gradient length of the text tower (include/mvlpt_hip.h: mvlpt_set_text_grad_len): text_bwd processes only the leading
        `grad_len` positions of every sequence; the rows behind a sequence's EOT carry an exactly zero gradient, so with
        grad_len > max_eot (the largest entry of the eot tables the caller is going to pass) the gradients keep their bits.
        grad_len = context_length: every position.  Applies from the next saving text forward."""
        _lib.check(lib.mvlpt_set_text_grad_len(self.h, int(grad_len), int(max_eot)), self.h, "set_text_grad_len")

    def set_text_shared_prefix(self, prefix: int) -> None:
        """Shared prefix of the class prompts (include/mvlpt_hip.h: mvlpt_set_text_shared_prefix): the caller vouches that the first
        `prefix` positions hold the same rows in every class (same layout columns, no suffix entry, one SOS embedding, a generic
        context, every EOT at or behind them); the next text forward evaluates them once and CONSUMES the setting (one-shot: the
        engine cannot check the claim against another call's tables).  0: off.  The engine lowers the value where its layout needs it
        and ignores it on the routes that have no shared layout."""
        _lib.check(lib.mvlpt_set_text_shared_prefix(self.h, int(prefix)), self.h, "set_text_shared_prefix")

    def text_act_ckpt_plan(self) -> List[Tuple[int, int, bool]]:
        """The plan the next saving text forward uses, as mvlpt_amd.model.checkpoint_segments gives it:
        [(first, last_exclusive, checkpointed)]."""
        layers = int(self.arch.transformer_layers)
        first, n = (C.c_int32 * max(layers, 1))(), C.c_int(0)
        _lib.check(lib.mvlpt_text_act_ckpt_plan(self.h, first, max(layers, 1), C.byref(n)), self.h, "text_act_ckpt_plan")
        lo = [int(first[i]) for i in range(n.value)] + [layers]
        return [(lo[i], lo[i + 1], i < n.value - 1) for i in range(n.value)]

    def set_vpt_dropout(self, masks: Optional[torch.Tensor]) -> None:
        """Per-image dropout masks of the visual prompt rows for the next image_fwd / image_bwd pair (include/mvlpt_hip.h:
        mvlpt_set_vpt_dropout): fp32 [n_layers, B, n_vpt, width], or None to clear.  One-shot: the next image_fwd consumes the setting
        (and keeps the tensor alive for its backward); a forward without a new call runs without dropout."""
        if self.resnet and masks is None:
            return      # nothing to clear: the tower takes no prompts
        self._refuse_on_resnet("visual prompt dropout")
        if masks is not None:
            masks = _req(masks, torch.float32, "vpt dropout masks")
            if masks.dim() != 4 or masks.shape[-1] != self.arch.vision_width:
                raise ValueError("vpt dropout masks must be [n_layers, B, n_vpt, vision_width]")
        self._vpt_masks = masks
        sh = (0, 0, 0, 0) if masks is None else tuple(int(v) for v in masks.shape)
        _lib.check(lib.mvlpt_set_vpt_dropout(self.h, _ptr(masks), *sh), self.h, "set_vpt_dropout")

    def _refuse_on_resnet(self, what: str) -> None:
        """The ResNet tower is frozen and runs forward-only in one piece; the reference cannot prompt it either
        (trainers/mvlpt.py:48 "HACK: Assume all is vision transformer")."""
        if self.resnet:
            raise ValueError(f"{what} is not available on a ResNet backbone ({self.arch.name}): the tower is frozen and forward-only "
                             "(the reference's trainers/mvlpt.py:48 assumes a vision transformer for visual prompts)")

    def debug_checksums(self, enable: bool = True):
        """mvlpt_debug_checksums: the stage fingerprints of the last image_fwd (list of ints) and the new on / off state."""
        buf = (C.c_uint64 * 256)()
        n = lib.mvlpt_debug_checksums(self.h, int(bool(enable)), buf, 256)
        if n < 0:
            raise RuntimeError(_lib.last_error(self.h))
        return [int(buf[i]) for i in range(n)]

    def set_ln_fold(self, mode: int, min_rows: int = 1024) -> None:
        """LayerNorm folding (include/mvlpt_hip.h: mvlpt_set_ln_fold): 0 off, 1 image tower, 2 both towers."""
        _lib.check(lib.mvlpt_set_ln_fold(self.h, int(mode), int(min_rows)), self.h, "set_ln_fold")

    def set_resid_packed(self, on: bool) -> None:
        """Packed residual stream of the prompt-free, gradient-free fp16 image tower (include/mvlpt_hip.h: mvlpt_set_resid_packed)."""
        _lib.check(lib.mvlpt_set_resid_packed(self.h, int(bool(on))), self.h, "set_resid_packed")

    @_on_device
    def trim(self) -> None:
        """Release workspace blocks that were outgrown (epoch boundary: synchronises the device)."""
        _lib.check(lib.mvlpt_trim(self.h), self.h, "trim")

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], compute_dtype: str = "fp16", device=None,
                        arch: Optional[ClipArch] = None, activation: str = "quick_gelu") -> "Engine":
        eng = cls(arch or arch_from_state_dict(sd), compute_dtype, device, activation)
        eng.load_frozen(sd)
        return eng

    def load_frozen(self, sd: Dict[str, torch.Tensor]) -> None:
        """Pack the frozen CLIP tensors (keys of clip.model.CLIP.state_dict())."""
        with torch.cuda.device(self.device):
            for name, t in sd.items():
                if name in ("logit_scale", "token_embedding.weight", "input_resolution", "context_length", "vocab_size"):
                    continue
                if name.endswith(".num_batches_tracked"):      # BatchNorm's step counter: not a weight
                    continue
                if t.dtype not in _TORCH2DT:
                    t = t.float()
                tg = t.to(self.device).contiguous()
                shape = (C.c_int64 * max(tg.dim(), 1))(*tg.shape)
                _lib.check(lib.mvlpt_load_frozen(self.h, name.encode(), _ptr(tg), _TORCH2DT[tg.dtype], shape, tg.dim(),
                                                 _stream()), self.h, f"load_frozen({name})")
                torch.cuda.current_stream().synchronize()   # tg may be freed right after
            _lib.check(lib.mvlpt_frozen_ready(self.h), self.h, "frozen_ready")

    # ------------------------------------------------------------------ towers
    def _image_args(self, image, vpt, vpt_deep):
        if image.dtype not in _TORCH2DT:
            image = image.float()
        image = image.contiguous()
        if not image.is_cuda:
            raise RuntimeError("image must be on the GPU")
        B = image.shape[0]
        n_vpt = n_deep = 0
        if vpt is not None:
            vpt = _req(vpt, torch.float32, "vpt").reshape(-1, self.arch.vision_width)
            n_vpt = vpt.shape[0]
        m = getattr(self, "_vpt_masks", None)
        if m is not None and (m.shape[1] != B or m.shape[2] != n_vpt):
            raise ValueError(f"vpt dropout masks are {tuple(m.shape)} but the batch has {B} images and {n_vpt} prompt tokens")
        if vpt_deep is not None:
            vpt_deep = _req(vpt_deep, torch.float32, "vpt_deep")
            n_deep = vpt_deep.shape[0]
        return image, vpt, vpt_deep, n_vpt, n_deep, B, m

    @_on_device
    def image_fwd(self, image: torch.Tensor, vpt: Optional[torch.Tensor] = None, vpt_deep: Optional[torch.Tensor] = None,
                  save_for_bwd: bool = False) -> torch.Tensor:
        if vpt is not None or vpt_deep is not None:
            self._refuse_on_resnet("visual prompts")
        if save_for_bwd:
            self._refuse_on_resnet("an image tower backward (save_for_bwd)")
        image, vpt, vpt_deep, n_vpt, n_deep, B, m = self._image_args(image, vpt, vpt_deep)
        feat = torch.empty(B, self.arch.embed_dim, device=image.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_image_fwd(self.h, _ptr(image), _TORCH2DT[image.dtype], _ptr(vpt), _ptr(vpt_deep), n_vpt, n_deep, B,
                                       _ptr(feat), int(save_for_bwd), _stream()), self.h, "image_fwd")
        self._img_state = (n_vpt, n_deep, B) if save_for_bwd else None
        # the setting was one-shot: this forward consumed it; its backward reads the buffer, so the tensor stays alive until then
        self._vpt_masks_saved, self._vpt_masks = (m if save_for_bwd else None), None
        return feat

    @_on_device
    def image_fwd_begin(self, image: torch.Tensor, vpt: Optional[torch.Tensor] = None, vpt_deep: Optional[torch.Tensor] = None,
                        save_for_bwd: bool = False, stop_block: Optional[int] = None) -> None:
        """First part of image_fwd on the current stream (mvlpt_image_fwd_begin): the tower entry and blocks [0, stop_block);
        None: everything ahead of the last block.  image_fwd_resume finishes the forward; the engine holds one pending forward."""
        self._refuse_on_resnet("image_fwd_begin / image_fwd_resume")
        image, vpt, vpt_deep, n_vpt, n_deep, B, m = self._image_args(image, vpt, vpt_deep)
        stop = self.arch.vision_layers if stop_block is None else int(stop_block)
        _lib.check(lib.mvlpt_image_fwd_begin(self.h, _ptr(image), _TORCH2DT[image.dtype], _ptr(vpt), _ptr(vpt_deep), n_vpt, n_deep, B,
                                             int(save_for_bwd), stop, _stream()), self.h, "image_fwd_begin")
        self._img_state = None
        # resume still reads the image-side inputs (deep prompts, masks): they stay alive until then
        self._img_pending = (image, vpt, vpt_deep, m, (n_vpt, n_deep, B) if save_for_bwd else None)
        self._vpt_masks = None

    @_on_device
    def image_fwd_resume(self) -> torch.Tensor:
        """Second part of the pending forward on the current stream (mvlpt_image_fwd_resume) -> features [B, embed] fp32.  The caller
        orders this stream behind the one image_fwd_begin ran on."""
        self._refuse_on_resnet("image_fwd_begin / image_fwd_resume")
        pend = self._img_pending
        if pend is None:
            raise RuntimeError("image_fwd_resume without image_fwd_begin")
        image, _vpt, _deep, m, state = pend
        feat = torch.empty(image.shape[0], self.arch.embed_dim, device=image.device, dtype=torch.float32)
        self._img_pending = None
        _lib.check(lib.mvlpt_image_fwd_resume(self.h, _ptr(feat), _stream()), self.h, "image_fwd_resume")
        self._img_state = state
        self._vpt_masks_saved = m if state is not None else None
        return feat

    def image_fwd_pending(self) -> bool:
        return self._img_pending is not None

    def image_fwd_abandon(self) -> None:
        """Forget a pending image_fwd_begin (mvlpt_image_fwd_abandon): host state only; the next begin reuses the workspace, so
        the caller orders it behind whatever the abandoned part enqueued."""
        _lib.check(lib.mvlpt_image_fwd_abandon(self.h), self.h, "image_fwd_abandon")
        self._img_pending = None

    @_on_device
    def image_bwd(self, dfeat: torch.Tensor) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        self._refuse_on_resnet("an image tower backward")
        if self._img_state is None:
            raise RuntimeError("image_bwd without image_fwd(save_for_bwd=True)")
        n_vpt, n_deep, B = self._img_state
        dfeat = _req(dfeat, torch.float32, "dfeat")
        dv = self.arch.vision_width
        dvpt = torch.empty(n_vpt, dv, device=dfeat.device, dtype=torch.float32) if n_vpt else None
        ddeep = torch.empty(n_deep, n_vpt, dv, device=dfeat.device, dtype=torch.float32) if n_deep else None
        _lib.check(lib.mvlpt_image_bwd(self.h, _ptr(dfeat), _ptr(dvpt), _ptr(ddeep), _stream()), self.h, "image_bwd")
        return dvpt, ddeep

    def _text_fwd(self, who, prefix, suffix, ctx, layout, eot, save_for_bwd, ctx_deep=None, ranges=None):
        """Every prompt forward (mvlpt_text_fwd): one MvlptTextJob, filled by field name.  ranges: _host_ranges' (lo, hi, S)."""
        prefix = _req(prefix, torch.float32, "token_prefix")
        suffix = _req(suffix, torch.float32, "token_suffix")
        layout = _req(layout, torch.int32, "layout")
        eot = _req(eot, torch.int32, "eot")
        rows, L = layout.shape
        job = _lib.MvlptTextJob(prefix=prefix.data_ptr(), suffix=suffix.data_ptr(), layout=layout.data_ptr(), eot=eot.data_ptr(),
                                n_cls=rows, L=L, save_for_bwd=int(save_for_bwd))
        if ctx is not None:
            ctx = _req(ctx, torch.float32, "ctx")
            job.ctx, job.n_ctx = ctx.data_ptr(), ctx.shape[-2]
        if ranges is not None:
            job.class_lo, job.class_hi, rows = ranges
            job.groups = ctx.shape[0]
        elif ctx is not None:
            job.ctx_per_class = int(ctx.dim() == 3)
        if ctx_deep is not None:
            ctx_deep = _req(ctx_deep, torch.float32, "ctx_deep")
            job.ctx_deep, job.n_deep = ctx_deep.data_ptr(), ctx_deep.shape[0]
        feat = torch.empty(rows, self.arch.embed_dim, device=prefix.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_text_fwd(self.h, C.byref(job), _ptr(feat), _stream()), self.h, who)
        self._txt_state = _TxtState(tuple(ctx.shape) if ctx is not None else None, layout, eot, ctx_deep,
                                    who == "text_fwd_deep") if save_for_bwd else None
        return feat

    @_on_device
    def text_fwd(self, prefix: torch.Tensor, suffix: torch.Tensor, ctx: Optional[torch.Tensor], layout: torch.Tensor,
                 eot: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        return self._text_fwd("text_fwd", prefix, suffix, ctx, layout, eot, save_for_bwd)

    @_on_device
    def text_fwd_deep(self, prefix: torch.Tensor, suffix: torch.Tensor, ctx: Optional[torch.Tensor], ctx_deep: Optional[torch.Tensor],
                      layout: torch.Tensor, eot: torch.Tensor, save_for_bwd: bool = False) -> torch.Tensor:
        """Deep language prompting (mvlpt_text_fwd with n_deep > 0): text_fwd with a generic ctx [n_ctx, dt] whose rows are replaced by
        ctx_deep[l - 1] ([n_deep, n_ctx, dt], 1 <= n_deep <= text_layers - 1) in front of block l.  ctx_deep None runs the plain tower
        (the bits of text_fwd).  A following text_bwd_deep returns (dctx, dctx_deep).  The engine reads ctx_deep again in a
        checkpointed backward; the tensor handed over here is kept until then."""
        if ctx is not None and ctx.dim() != 2:
            raise ValueError("deep text prompts take a generic ctx [n_ctx, ctx_dim] (no per-class contexts)")
        n_ctx = ctx.shape[0] if ctx is not None else 0
        if ctx_deep is not None and (ctx_deep.dim() != 3 or ctx_deep.shape[1] != n_ctx or ctx_deep.shape[2] != self.arch.transformer_width):
            raise ValueError(f"ctx_deep must be [n_deep, {n_ctx}, {self.arch.transformer_width}], got {tuple(ctx_deep.shape)}")
        return self._text_fwd("text_fwd_deep", prefix, suffix, ctx, layout, eot, save_for_bwd, ctx_deep=ctx_deep)

    @_on_device
    def text_fwd_ranged(self, prefix: torch.Tensor, suffix: torch.Tensor, ctx: torch.Tensor, layout: torch.Tensor, eot: torch.Tensor,
                        class_lo, class_hi, save_for_bwd: bool = False) -> torch.Tensor:
        """The ranged text side (mvlpt_text_fwd with class ranges): ctx [G, n_ctx, dt]; image g runs classes [class_lo[g], class_hi[g]) only.
        `class_lo` / `class_hi` are HOST integer sequences (lists, numpy or CPU tensors) of length G: nothing is read back from the
        device.  Features [S, e], S = sum of the range widths, group after group.  A following text_bwd returns [G, n_ctx, dt].
        [0] * G, [C] * G is CoCoOp's text side: features [G*C, e], row g*C + c = (image g, class c)."""
        if ctx.dim() != 3:
            raise ValueError("ranged ctx must be [G, n_ctx, ctx_dim]")
        ranges = _host_ranges(class_lo, class_hi, ctx.shape[0], layout.shape[0])
        return self._text_fwd("text_fwd_ranged", prefix, suffix, ctx, layout, eot, save_for_bwd, ranges=ranges)

    def load_token_embedding(self, weight: torch.Tensor) -> None:
        """Opt-in: keep an fp32 copy of `token_embedding.weight` [vocab, text_width] on the device for text_encode_tokens
        (load_frozen skips the key, so the prompt-tuning routes never pay for it)."""
        with torch.cuda.device(self.device):
            tg = weight.detach().float().to(self.device).contiguous()
            if tg.dim() != 2 or tg.shape[1] != self.arch.transformer_width:
                raise ValueError(f"token_embedding.weight must be [vocab, {self.arch.transformer_width}], got {tuple(tg.shape)}")
            shape = (C.c_int64 * 2)(*tg.shape)
            _lib.check(lib.mvlpt_load_frozen(self.h, b"token_embedding.weight", _ptr(tg), DT_F32, shape, 2, _stream()), self.h,
                       "load_frozen(token_embedding.weight)")
            torch.cuda.current_stream().synchronize()   # tg may be freed right after
        self.vocab_size = int(tg.shape[0])

    @_on_device
    def text_encode_tokens(self, ids, L: Optional[int] = None) -> torch.Tensor:
        """CLIP.encode_text over token ids (mvlpt_text_encode_tokens): `ids` is a HOST integer array [S, ld] (CPU tensor or numpy);
        the tower runs the first L columns (default: all of them).  Un-normalised features [S, embed] fp32 on the device."""
        if isinstance(ids, torch.Tensor):
            if ids.is_cuda:
                raise ValueError("token ids are a host array (they are checked on the host and uploaded with the call)")
            ids = ids.numpy()
        import numpy as np
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2:
            raise ValueError("token ids must be [S, ld]")
        S, ld = ids.shape
        L = ld if L is None else int(L)
        feat = torch.empty(S, self.arch.embed_dim, device=self.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_text_encode_tokens(self.h, C.c_void_p(ids.ctypes.data), ld, S, L, _ptr(feat), _stream()), self.h,
                   "text_encode_tokens")
        self._txt_state = None
        return feat

    @_on_device
    def nearest_tokens(self, q: torch.Tensor, k: int, max_rows: int = _lib.NEAREST_MAX_ROWS) -> Tuple[torch.Tensor, torch.Tensor]:
        """The k nearest rows of the resident token table for every row of q [R, text_width] (mvlpt_nearest_tokens): token ids int64
        [R, k] and Euclidean distances fp32 [R, k], ascending by (distance, id), on the device.  No [R, vocab] matrix is built.  The
        table is uploaded on first use (FrozenCLIP's loader, the one encode_text uses).  R above `max_rows` (the grid's limit,
        MVLPT_NEAREST_MAX_ROWS) runs in chunks of that many rows; the rows are independent, so chunking changes no result."""
        q = _req(q, torch.float32, "q")
        if q.dim() != 2 or q.shape[0] == 0 or q.shape[1] != self.arch.transformer_width:
            raise ValueError(f"q must be [R >= 1, {self.arch.transformer_width}], got {tuple(q.shape)}")
        k = int(k)
        if not 1 <= k <= _lib.NEAREST_MAX_K:
            raise ValueError(f"topk must lie in [1, {_lib.NEAREST_MAX_K}] (MVLPT_NEAREST_MAX_K), got {k}")
        if not 1 <= max_rows <= _lib.NEAREST_MAX_ROWS:
            raise ValueError(f"max_rows must lie in [1, {_lib.NEAREST_MAX_ROWS}]")
        load = self.token_table_loader() if self.token_table_loader is not None else None
        if load is not None:
            load()
        R = q.shape[0]
        idx = torch.empty(R, k, device=q.device, dtype=torch.int32)
        dist = torch.empty(R, k, device=q.device, dtype=torch.float32)
        for r0 in range(0, R, max_rows):
            r1 = min(R, r0 + max_rows)
            _lib.check(lib.mvlpt_nearest_tokens(self.h, _ptr(q[r0:r1]), r1 - r0, k, _ptr(idx[r0:r1]), _ptr(dist[r0:r1]), _stream()),
                       self.h, "nearest_tokens")
        return idx.long(), dist

    def text_encode_workspace_bytes(self, n_seq: int, L: int) -> int:
        """Workspace text_encode_tokens reserves for `n_seq` sequences of length L: the tower's plus the id table (include/mvlpt_hip.h)."""
        return self.text_workspace_bytes(n_seq, L, False) + ((4 * (n_seq * L + n_seq) + 255) & ~255)

    def text_ensemble(self, feats: torch.Tensor) -> torch.Tensor:
        """Prompt ensembling (mvlpt_text_ensemble): feats [T, C, e] fp32, template-major -> [C, e] unit rows."""
        feats = _req(feats, torch.float32, "feats")
        if feats.dim() != 3:
            raise ValueError("feats must be [T, C, embed]")
        T, Cn, e = feats.shape
        out = torch.empty(Cn, e, device=feats.device, dtype=torch.float32)
        with torch.cuda.device(feats.device):
            _lib.check(lib.mvlpt_text_ensemble(_ptr(feats), T, Cn, e, _ptr(out), _stream()), None, "text_ensemble")
        return out

    def text_workspace_bytes(self, n_seq: int, L: int, save_for_bwd: bool) -> int:
        """Text-tower workspace a forward over `n_seq` sequences of length L reserves (mvlpt_text_workspace_bytes)."""
        out = C.c_int64()
        _lib.check(lib.mvlpt_text_workspace_bytes(self.h, int(n_seq), int(L), int(save_for_bwd), C.byref(out)), self.h,
                   "text_workspace_bytes")
        return int(out.value)

    def _text_bwd(self, who: str, dfeat: torch.Tensor, deep: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        st = self._txt_state
        if st is None or st.ctx_shape is None or (deep and not st.deep):
            raise RuntimeError(f"{who} without {'text_fwd_deep' if deep else 'text_fwd'}(save_for_bwd=True) with context tokens")
        dfeat = _req(dfeat, torch.float32, "dfeat")
        dctx = torch.empty(st.ctx_shape, device=dfeat.device, dtype=torch.float32)
        ddeep = torch.empty_like(st.ctx_deep) if deep and st.ctx_deep is not None else None
        _lib.check(lib.mvlpt_text_bwd(self.h, _ptr(dfeat), _ptr(dctx), _ptr(ddeep), _stream()), self.h, who)
        return dctx, ddeep

    @_on_device
    def text_bwd(self, dfeat: torch.Tensor) -> torch.Tensor:
        return self._text_bwd("text_bwd", dfeat, False)[0]

    @_on_device
    def text_bwd_deep(self, dfeat: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(dctx, dctx_deep) of the last text_fwd_deep(save_for_bwd=True); dctx_deep is None when that forward had no deep prompts."""
        return self._text_bwd("text_bwd_deep", dfeat, True)

    # ------------------------------------------------------------------ head
    @_on_device
    def logits_fwd(self, img_feat, txt_feat, logit_scale_exp: float, task_lo=None, task_hi=None) -> torch.Tensor:
        img_feat = _req(img_feat, torch.float32, "img_feat")
        txt_feat = _req(txt_feat, torch.float32, "txt_feat")
        if task_lo is not None:
            task_lo = _req(task_lo, torch.int32, "task_lo")
            task_hi = _req(task_hi, torch.int32, "task_hi")
        B, Cn = img_feat.shape[0], txt_feat.shape[0]
        logits = torch.empty(B, Cn, device=img_feat.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_logits_fwd(self.h, _ptr(img_feat), _ptr(txt_feat), float(logit_scale_exp), _ptr(task_lo),
                                        _ptr(task_hi), B, Cn, _ptr(logits), _stream()), self.h, "logits_fwd")
        self._head_state = (task_lo, task_hi, B, Cn)   # keep the mask tensors alive until logits_bwd
        return logits

    @_on_device
    def logits_bwd(self, dlogits, need_img: bool = True, need_txt: bool = True):
        if self._head_state is None:
            raise RuntimeError("logits_bwd without logits_fwd")
        _, _, B, Cn = self._head_state
        dlogits = _req(dlogits, torch.float32, "dlogits")
        e = self.arch.embed_dim
        dimg = torch.empty(B, e, device=dlogits.device, dtype=torch.float32) if need_img else None
        dtxt = torch.empty(Cn, e, device=dlogits.device, dtype=torch.float32) if need_txt else None
        _lib.check(lib.mvlpt_logits_bwd(self.h, _ptr(dlogits), _ptr(dimg), _ptr(dtxt), _stream()), self.h, "logits_bwd")
        return dimg, dtxt

    @_on_device
    def logits_ranged_fwd(self, img_feat, txt_feat, logit_scale_exp: float, class_lo, class_hi, n_cls: int) -> torch.Tensor:
        """The ranged head (mvlpt_logits_ranged_fwd): img [G, e] against txt [S, e] (rows of text_fwd_ranged over the same host ranges)
        -> logits [G, n_cls], exactly 0 outside image g's range.  [0] * G, [C] * G is CoCoOp's head: img [G, e] against its own
        rows of txt [G*C, e]."""
        img_feat = _req(img_feat, torch.float32, "img_feat")
        txt_feat = _req(txt_feat, torch.float32, "txt_feat")
        G = img_feat.shape[0]
        lo, hi, S = _host_ranges(class_lo, class_hi, G, n_cls)
        if txt_feat.shape[0] != S:
            raise ValueError(f"ranged head: {txt_feat.shape[0]} text rows but the ranges hold {S} sequences")
        logits = torch.empty(G, n_cls, device=img_feat.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_logits_ranged_fwd(self.h, _ptr(img_feat), _ptr(txt_feat), float(logit_scale_exp), lo, hi, G, n_cls,
                                               _ptr(logits), _stream()), self.h, "logits_ranged_fwd")
        self._head_state = (None, None, G, S)
        return logits

    @_on_device
    def logits_ranged_bwd(self, dlogits, need_img: bool = False, need_txt: bool = True):
        """(d img [G, e] w.r.t. the un-normalised image features or None, d txt [S, e] or None) of the last logits_ranged_fwd."""
        if self._head_state is None:
            raise RuntimeError("logits_ranged_bwd without logits_ranged_fwd")
        _, _, G, S = self._head_state
        dlogits = _req(dlogits, torch.float32, "dlogits")
        e = self.arch.embed_dim
        dimg = torch.empty(G, e, device=dlogits.device, dtype=torch.float32) if need_img else None
        dtxt = torch.empty(S, e, device=dlogits.device, dtype=torch.float32) if need_txt else None
        _lib.check(lib.mvlpt_logits_ranged_bwd(self.h, _ptr(dlogits), _ptr(dtxt), _ptr(dimg), _stream()), self.h, "logits_ranged_bwd")
        return dimg, dtxt

    @_on_device
    def tpt_head_fwd(self, img, txt, logit_scale_exp: float, k: int, want_logits: bool = False):
        """The test-time prompt tuning head (mvlpt_op_tpt_head_fwd): img [G, V, e] views against txt [G*C, e] (rows of text_fwd_ranged
        over full ranges) -> (loss [G], H [G, V], sel int32 [G, k]), and z [G, V, C] as a fourth value under `want_logits` (tests).
        Device tensors, no host sync.  The workspace is the engine's own, grow-only; tpt_head_bwd reads it."""
        self._tpt_state = None
        img = _req(img, torch.float32, "img")
        txt = _req(txt, torch.float32, "txt")
        if img.dim() != 3 or txt.dim() != 2 or img.shape[2] != txt.shape[1]:
            raise ValueError("tpt head: img must be [G, V, e] and txt [G*C, e]")
        G, V, e = img.shape
        if G == 0 or txt.shape[0] == 0 or txt.shape[0] % G:
            raise ValueError(f"tpt head: {txt.shape[0]} text rows are not a whole number of classes for each of {G} images")
        Cn, k = txt.shape[0] // G, int(k)
        nb = C.c_int64()
        _lib.check(lib.mvlpt_tpt_workspace_bytes(G, V, Cn, e, k, C.byref(nb)), None, "tpt_workspace_bytes")
        ws = getattr(self, "_tpt_ws", None)
        if ws is None or ws.numel() * 8 < nb.value or ws.device != img.device:
            ws = self._tpt_ws = torch.empty((nb.value + 7) // 8, device=img.device, dtype=torch.int64)
        loss = torch.empty(G, device=img.device, dtype=torch.float32)
        H = torch.empty(G, V, device=img.device, dtype=torch.float32)
        sel = torch.empty(G, k, device=img.device, dtype=torch.int32)
        z = torch.empty(G, V, Cn, device=img.device, dtype=torch.float32) if want_logits else None
        _lib.check(lib.mvlpt_op_tpt_head_fwd(_ptr(img), _ptr(txt), float(logit_scale_exp), G, V, Cn, e, k, _ptr(loss), _ptr(H), _ptr(sel),
                                             _ptr(z), _ptr(ws), ws.numel() * 8, _stream()), None, "op_tpt_head_fwd")
        self._tpt_state = (float(logit_scale_exp), G, V, Cn, e, k)
        return (loss, H, sel, z) if want_logits else (loss, H, sel)

    @_on_device
    def tpt_head_bwd(self, weights=None) -> torch.Tensor:
        """d (sum_g weights[g] * loss[g]) / d txt [G*C, e] of the last tpt_head_fwd (selection constant; weights None: all 1)."""
        if getattr(self, "_tpt_state", None) is None:
            raise RuntimeError("tpt_head_bwd without tpt_head_fwd")
        scale, G, V, Cn, e, k = self._tpt_state
        ws = self._tpt_ws
        if weights is not None:
            weights = _req(weights, torch.float32, "weights")
            if weights.shape != (G,):
                raise ValueError(f"tpt head: weights must be [{G}]")
        dtxt = torch.empty(G * Cn, e, device=ws.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_op_tpt_head_bwd(_ptr(weights), scale, G, V, Cn, e, k, _ptr(dtxt), _ptr(ws), ws.numel() * 8, _stream()),
                   None, "op_tpt_head_bwd")
        return dtxt

    # ---- Tip-Adapter head (mvlpt_op_tip_*): F [N, D] unit features, K [NK, D] keys sorted by class, key_ptr int32 [C + 1], W [C, D]
    def _tip_args(self, F, K, key_ptr, W):
        F, K, W = _req(F, torch.float32, "F"), _req(K, torch.float32, "K"), _req(W, torch.float32, "W")
        key_ptr = _req(key_ptr, torch.int32, "key_ptr")
        if F.dim() != 2 or K.dim() != 2 or W.dim() != 2 or K.shape[1] != F.shape[1] or W.shape[1] != F.shape[1]:
            raise ValueError("tip head: F must be [N, D], K [NK, D] and W [C, D]")
        if key_ptr.shape != (W.shape[0] + 1,):
            raise ValueError(f"tip head: key_ptr must be [{W.shape[0] + 1}]")
        return F, K, key_ptr, W, (F.shape[0], K.shape[0], W.shape[0], F.shape[1])

    def _tip_workspace(self, N, NK, Cn, D, nb, na, mode, device):
        need = C.c_int64()
        _lib.check(lib.mvlpt_tip_workspace_bytes(N, NK, Cn, D, nb, na, mode, C.byref(need)), None, "tip_workspace_bytes")
        ws = getattr(self, "_tip_ws", None)
        if ws is None or ws.numel() * 8 < need.value or ws.device != device:
            ws = self._tip_ws = torch.empty((need.value + 7) // 8, device=device, dtype=torch.int64)
        return ws

    @_on_device
    def tip_logits(self, F, K, key_ptr, W, logit_scale_exp: float, alpha: float, beta: float) -> torch.Tensor:
        """logits [N, C] = s F W^T + alpha * (per-class sums of exp(-beta (1 - F K^T))) (mvlpt_op_tip_logits).  No host sync."""
        F, K, key_ptr, W, (N, NK, Cn, D) = self._tip_args(F, K, key_ptr, W)
        logits = torch.empty(N, Cn, device=F.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_op_tip_logits(_ptr(F), _ptr(K), _ptr(key_ptr), _ptr(W), float(logit_scale_exp), float(alpha), float(beta),
                                           N, NK, Cn, D, _ptr(logits), _stream()), None, "op_tip_logits")
        return logits

    @_on_device
    def tip_train_fwd(self, F, y, K, key_ptr, W, logit_scale_exp: float, alpha: float, beta: float, want_logits: bool = False):
        """(loss [1], correct int32 [1]) of the Tip-Adapter-F step, and the logits [N, C] as a third value under `want_logits`
        (mvlpt_op_tip_train_fwd).  The workspace is the engine's own, grow-only; tip_train_bwd reads it."""
        self._tip_state = None
        F, K, key_ptr, W, (N, NK, Cn, D) = self._tip_args(F, K, key_ptr, W)
        y = _req(y, torch.int32, "y")
        if y.shape != (N,):
            raise ValueError(f"tip head: y must be [{N}]")
        ws = self._tip_workspace(N, NK, Cn, D, 0, 0, _lib.TIP_TRAIN, F.device)
        loss = torch.empty(1, device=F.device, dtype=torch.float32)
        correct = torch.empty(1, device=F.device, dtype=torch.int32)
        logits = torch.empty(N, Cn, device=F.device, dtype=torch.float32) if want_logits else None
        _lib.check(lib.mvlpt_op_tip_train_fwd(_ptr(F), _ptr(y), _ptr(K), _ptr(key_ptr), _ptr(W), float(logit_scale_exp), float(alpha),
                                              float(beta), N, NK, Cn, D, _ptr(loss), _ptr(correct), _ptr(logits), _ptr(ws),
                                              ws.numel() * 8, _stream()), None, "op_tip_train_fwd")
        self._tip_state = (F, float(alpha), float(beta), N, NK, Cn, D)
        return (loss, correct, logits) if want_logits else (loss, correct)

    @_on_device
    def tip_train_bwd(self) -> torch.Tensor:
        """d loss / d K [NK, D] of the last tip_train_fwd."""
        if getattr(self, "_tip_state", None) is None:
            raise RuntimeError("tip_train_bwd without tip_train_fwd")
        F, alpha, beta, N, NK, Cn, D = self._tip_state
        ws = self._tip_ws
        dK = torch.empty(NK, D, device=F.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_op_tip_train_bwd(_ptr(F), alpha, beta, N, NK, Cn, D, _ptr(dK), _ptr(ws), ws.numel() * 8, _stream()),
                   None, "op_tip_train_bwd")
        return dK

    @_on_device
    def tip_search(self, F, y, K, key_ptr, W, logit_scale_exp: float, betas, alphas) -> torch.Tensor:
        """counts int32 [nb, na]: the rows whose arg-max at (betas[b], alphas[a]) is y (mvlpt_op_tip_search).  It uses the workspace
        of the train entries: a tip_train_fwd before it can no longer be followed by tip_train_bwd."""
        self._tip_state = None
        F, K, key_ptr, W, (N, NK, Cn, D) = self._tip_args(F, K, key_ptr, W)
        y = _req(y, torch.int32, "y")
        betas, alphas = _req(betas, torch.float32, "betas"), _req(alphas, torch.float32, "alphas")
        if y.shape != (N,) or betas.dim() != 1 or alphas.dim() != 1:
            raise ValueError(f"tip head: y must be [{N}], betas and alphas vectors")
        nb, na = betas.shape[0], alphas.shape[0]
        ws = self._tip_workspace(N, NK, Cn, D, nb, na, _lib.TIP_SEARCH, F.device)
        counts = torch.empty(nb, na, device=F.device, dtype=torch.int32)
        _lib.check(lib.mvlpt_op_tip_search(_ptr(F), _ptr(y), _ptr(K), _ptr(key_ptr), _ptr(W), float(logit_scale_exp), _ptr(betas),
                                           _ptr(alphas), N, NK, Cn, D, nb, na, _ptr(counts), _ptr(ws), ws.numel() * 8, _stream()),
                   None, "op_tip_search")
        return counts

    @_on_device
    def cross_entropy(self, logits, label, need_grad: bool = True):
        """Returns (loss[1], dlogits or None, ncorrect[1]) — device tensors, no host sync."""
        logits = _req(logits, torch.float32, "logits")
        B, Cn = logits.shape
        if label.dtype in (torch.int64, torch.int32, torch.int16, torch.uint8):
            label = _req(label, torch.int64, "label")
            kind = _lib.LABEL_INT64
            if label.shape != (B,):
                raise ValueError("integer labels must have shape [B]")
        else:
            label = _req(label, torch.float32, "label")
            kind = _lib.LABEL_PROB_F32
            if label.shape != (B, Cn):
                raise ValueError("probability labels must have shape [B, C]")
        loss = torch.empty(1, device=logits.device, dtype=torch.float32)
        nc = torch.empty(1, device=logits.device, dtype=torch.float32)
        dl = torch.empty_like(logits) if need_grad else None
        _lib.check(lib.mvlpt_cross_entropy(self.h, _ptr(logits), _ptr(label), kind, B, Cn, _ptr(loss), _ptr(dl), _ptr(nc),
                                           _stream()), self.h, "cross_entropy")
        return loss, dl, nc

    # ------------------------------------------------------------------ input pipeline
    @_on_device
    def preprocess(self, src: torch.Tensor, descs, out_size, mean, std, out_dtype=torch.float32, want_u8: bool = False):
        """src: uint8 device tensor holding the packed decoded HWC images; descs: `_lib.MvlptImageDesc` ctypes array.
        Returns [B,3,h,w] normalised images (and the resized 8-bit images [B,h,w,3] when `want_u8`)."""
        if not src.is_cuda or src.dtype != torch.uint8:
            raise RuntimeError("src must be a uint8 CUDA/HIP tensor: mvlpt_amd has no CPU path")
        src = src.contiguous()
        B = len(descs)
        oh, ow = (out_size, out_size) if isinstance(out_size, int) else tuple(out_size)
        out = torch.empty(B, 3, oh, ow, device=src.device, dtype=out_dtype)
        u8 = torch.empty(B, oh, ow, 3, device=src.device, dtype=torch.uint8) if want_u8 else None
        m = (C.c_float * 3)(*[float(v) for v in mean])
        sd = (C.c_float * 3)(*[float(v) for v in std])
        _lib.check(lib.mvlpt_preprocess(self.h, _ptr(src), src.numel(), descs, B, oh, ow, m, sd, _ptr(out), _TORCH2DT[out_dtype],
                                        _ptr(u8), _stream()), self.h, "preprocess")
        return (out, u8) if want_u8 else out

    @_on_device
    def preprocess_aug(self, src: torch.Tensor, descs, augs, out_size, mean, std, out_dtype=torch.float32, want_u8: bool = False,
                       fill_outside: bool = False):
        """`preprocess` with the augmentations of `mvlpt_preprocess_aug`: augs is a `_lib.MvlptAugmentDesc` ctypes array (one per image:
        colour operations, grayscale, cutout holes) or None; fill_outside lets a window hang over the resized image, zero filled
        (random_crop with padding).  The 8-bit images of `want_u8` are the ones just before ToTensor, after every augmentation."""
        if not src.is_cuda or src.dtype != torch.uint8:
            raise RuntimeError("src must be a uint8 CUDA/HIP tensor: mvlpt_amd has no CPU path")
        if augs is not None and len(augs) != len(descs):
            raise ValueError("one augmentation descriptor per image descriptor")
        src = src.contiguous()
        B = len(descs)
        oh, ow = (out_size, out_size) if isinstance(out_size, int) else tuple(out_size)
        out = torch.empty(B, 3, oh, ow, device=src.device, dtype=out_dtype)
        u8 = torch.empty(B, oh, ow, 3, device=src.device, dtype=torch.uint8) if want_u8 else None
        m = (C.c_float * 3)(*[float(v) for v in mean])
        sd = (C.c_float * 3)(*[float(v) for v in std])
        _lib.check(lib.mvlpt_preprocess_aug(self.h, _ptr(src), src.numel(), descs, augs, B, oh, ow, int(bool(fill_outside)), m, sd,
                                            _ptr(out), _TORCH2DT[out_dtype], _ptr(u8), _stream()), self.h, "preprocess_aug")
        return (out, u8) if want_u8 else out

    # ------------------------------------------------------------------ profiling
    @_on_device
    def profile_begin(self, all_kernels: bool = False):
        _lib.check(lib.mvlpt_profile_begin(self.h, int(all_kernels)), self.h, "profile_begin")

    @_on_device
    def profile_pause(self, paused: bool):
        _lib.check(lib.mvlpt_profile_pause(self.h, int(paused)), self.h, "profile_pause")

    @_on_device
    def profile_end(self) -> Dict[str, dict]:
        arr = (_lib.MvlptKernelStat * 64)()
        n = lib.mvlpt_profile_end(self.h, arr, 64)
        if n < 0:
            raise RuntimeError("profile_end failed")
        return {arr[i].name.decode(): dict(launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops, bytes=arr[i].bytes,
                                           busy_ms=arr[i].busy_ms, flops_executed=arr[i].flops_executed)
                for i in range(n)}


# ---------------------------------------------------------------------- kernel-level ops (parity tests)
def op_gemm(A, Bt, epi=_lib.EPI_STORE16, bias=None, aux=None, resid=None, out2=False):
    dt = _TORCH2DT[A.dtype]
    M, K = A.shape
    N = Bt.shape[0]
    out_dtype = torch.float32 if epi in (_lib.EPI_RESID32, _lib.EPI_STORE32) else A.dtype
    out = torch.empty(M, N, device=A.device, dtype=out_dtype)
    o2 = torch.empty(M, N, device=A.device, dtype=A.dtype) if out2 else None
    _lib.check(lib.mvlpt_op_gemm(dt, epi, _ptr(A.contiguous()), _ptr(Bt.contiguous()), M, N, K, _ptr(bias), _ptr(aux),
                                 _ptr(resid), _ptr(out), _ptr(o2), _stream()), None, "op_gemm")
    return (out, o2) if out2 else out


def op_gemm_ex(A, Bt, epi, M, N, K, out, bias=None, aux=None, resid=None, out2=None, a_split=0, lda=0, ldo=0, ldb=0, w8_exp=0, out_lo8=0):
    """mvlpt_op_gemm_ex on caller-owned tensors (nothing is copied or made contiguous: pitches and aliasing are the caller's)."""
    _lib.check(lib.mvlpt_op_gemm_ex(_TORCH2DT[A.dtype], epi, _ptr(A), _ptr(Bt), M, N, K, _ptr(bias), _ptr(aux), _ptr(resid), _ptr(out),
                                    _ptr(out2), a_split, lda, ldo, ldb, w8_exp, out_lo8, _stream()), None, "op_gemm_ex")
    return out


def _act_code(activation) -> int:
    return _ACTIVATIONS.get(activation, activation)


def op_activation_fwd(u32, M, N, out, activation="gelu", out_format=0, ld_in=0, ld_out=0, u16_out=None):
    """mvlpt_op_activation_fwd on caller-owned tensors: out (16-bit, format _lib.ACT_OUT_*, pitch ld_out) = act(u32 fp32 [M, N] at
    pitch ld_in); u16_out (optional, [M, N]): the saved pre-activation.  `activation`: "quick_gelu" | "gelu" (or a raw code)."""
    _lib.check(lib.mvlpt_op_activation_fwd(_TORCH2DT[out.dtype], _act_code(activation), _ptr(u32), ld_in, M, N, out_format, _ptr(out),
                                           ld_out, _ptr(u16_out), _stream()), None, "op_activation_fwd")
    return out


def op_activation_bwd(da32, u16, M, N, out, activation="gelu", out_format=0, ld_in=0, ld_out=0):
    """mvlpt_op_activation_bwd: out = da32 (fp32 [M, N] at pitch ld_in) * act'(u16 [M, N]) in format out_format at pitch ld_out."""
    _lib.check(lib.mvlpt_op_activation_bwd(_TORCH2DT[out.dtype], _act_code(activation), _ptr(da32), ld_in, _ptr(u16), M, N, out_format,
                                           _ptr(out), ld_out, _stream()), None, "op_activation_bwd")
    return out


Engine.op_activation_fwd = staticmethod(op_activation_fwd)
Engine.op_activation_bwd = staticmethod(op_activation_bwd)


def op_gemm_route(dtype, epi, a_split, M, N, K, fold_ntp=0):
    """(family, tile_m, tile_n, ring depth) of the kernel a GEMM on the current stream would use (_lib.GEMM_*)."""
    tm, tn, ring = C.c_int(0), C.c_int(0), C.c_int(0)
    fam = lib.mvlpt_op_gemm_route(_TORCH2DT[dtype], epi, a_split, M, N, K, fold_ntp, _stream(), C.byref(tm), C.byref(tn), C.byref(ring))
    if fam <= 0:
        raise RuntimeError(f"libmvlpt_hip op_gemm_route failed (code {fam}): {_lib.last_error(None)}")
    return fam, tm.value, tn.value, ring.value


def split_pair(x: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 [M,K] -> 16-bit hi|lo pair [M,2K] (the layout of GemmArgs::a_split; host-side helper for tests)."""
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    return torch.cat([hi, lo], dim=1).contiguous()


def join_pair(p: torch.Tensor) -> torch.Tensor:
    k = p.shape[1] // 2
    return p[:, :k].float() + p[:, k:].float()


def op_gemm_split(A2, Bt, epi=_lib.EPI_STORE32, bias=None, aux=None, resid=None, out2=False):
    """A2: 16-bit pair [M,2K]."""
    dt = _TORCH2DT[A2.dtype]
    M, K = A2.shape[0], A2.shape[1] // 2
    N = Bt.shape[0]
    if epi in (_lib.EPI_RESID32, _lib.EPI_STORE32):
        out = torch.empty(M, N, device=A2.device, dtype=torch.float32)
    elif epi in (_lib.EPI_GELU_SPLIT, _lib.EPI_GELUBWD_SPLIT, _lib.EPI_STORE_SPLIT):
        out = torch.empty(M, 2 * N, device=A2.device, dtype=A2.dtype)
    else:
        out = torch.empty(M, N, device=A2.device, dtype=A2.dtype)
    o2 = torch.empty(M, N, device=A2.device, dtype=A2.dtype) if out2 else None
    _lib.check(lib.mvlpt_op_gemm_split(dt, epi, _ptr(A2.contiguous()), _ptr(Bt.contiguous()), M, N, K, _ptr(bias), _ptr(aux),
                                       _ptr(resid), _ptr(out), _ptr(o2), _stream()), None, "op_gemm_split")
    return (out, o2) if out2 else out


# ---- mixed pair: [hi (d x 16 bit) | residual bytes (d, e5m2 of (x - hi) * 2^LO8_EXP) | unused], pitch 2d 16-bit elements
LO8_EXP = {torch.float16: 10, torch.bfloat16: 7}


def join_mixed(p: torch.Tensor) -> torch.Tensor:
    """Value of a mixed-pair tensor [rows, 2d] (host-side decoder for tests)."""
    d = p.shape[1] // 2
    lo8 = p[:, d:d + d // 2].contiguous().view(torch.uint8).view(torch.float8_e5m2).float()
    return p[:, :d].float() + lo8 * 2.0 ** -LO8_EXP[p.dtype]


def op_assemble_prompts_ranged(prefix, suffix, ctx, layout, pos, class_lo, class_hi) -> torch.Tensor:
    """x [S, L, d] of the ranged tower's entry (mvlpt_op_assemble_prompts_ranged): class rows of prefix [C,1,d] / suffix [C,L-1-n,d] /
    layout [C,L] with context block g of ctx [G,n,d], plus pos [L,d] (the first L rows are read).  class_lo / class_hi: host sequences
    of length G; [0]*G, [C]*G is CoCoOp's tower, S = G*C."""
    G, n, d = ctx.shape
    C_, L = layout.shape
    lo, hi, S = _host_ranges(class_lo, class_hi, G, C_)
    x = torch.empty(S, L, d, device=ctx.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_assemble_prompts_ranged(_ptr(prefix.contiguous()), _ptr(suffix.contiguous()), _ptr(ctx.contiguous()), n,
                                                    _ptr(layout.to(torch.int32).contiguous()), _ptr(pos.contiguous()), _ptr(x),
                                                    lo, hi, G, C_, L, d, _stream()), None, "op_assemble_prompts_ranged")
    return x


def op_gather_ctx_grad_ranged(dx, ctx_pos, class_lo, class_hi) -> torch.Tensor:
    """dctx [G, n_ctx, d] from dx [S, L, d] and ctx_pos [C, n_ctx] (mvlpt_op_gather_ctx_grad_ranged)."""
    S_, L, d = dx.shape
    C_, n = ctx_pos.shape
    G = len(class_lo)
    lo, hi, S = _host_ranges(class_lo, class_hi, G, C_)
    if S != S_:
        raise ValueError(f"dx has {S_} sequences but the ranges hold {S}")
    dctx = torch.empty(G, n, d, device=dx.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_gather_ctx_grad_ranged(_ptr(dx.contiguous()), _ptr(ctx_pos.to(torch.int32).contiguous()), lo, hi, G, C_, L, d,
                                                   n, _ptr(dctx), _stream()), None, "op_gather_ctx_grad_ranged")
    return dctx


def op_embed_tokens(emb, pos, ids, L: int, out=None) -> torch.Tensor:
    """x [S, L, d] = emb[ids[:, :L]] + pos[:L] (the entry of mvlpt_text_encode_tokens); ids int32 [S, ld] on the DEVICE, only columns
    0 .. L-1 are read and must be rows of emb.  `out`: a preallocated buffer whose first S * L * d floats are written."""
    emb, pos, ids = _req(emb, torch.float32, "emb"), _req(pos, torch.float32, "pos"), _req(ids, torch.int32, "ids")
    S, ld = ids.shape
    d = emb.shape[1]
    x = out if out is not None else torch.empty(S, L, d, device=emb.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_embed_tokens(_ptr(emb), _ptr(pos), _ptr(ids), ld, _ptr(x), S, int(L), d, _stream()), None, "op_embed_tokens")
    return x


def nearest_workspace_bytes(R: int, V: int, d: int, k: int) -> int:
    """Scratch bytes op_nearest_rows needs for these sizes on the current stream (mvlpt_nearest_workspace_bytes)."""
    out = C.c_int64()
    _lib.check(lib.mvlpt_nearest_workspace_bytes(int(R), int(V), int(d), int(k), _stream(), C.byref(out)), None, "nearest_workspace_bytes")
    return int(out.value)


def op_nearest_rows(q, table, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx int32 [R, k], dist fp32 [R, k]): the k nearest rows of table [V, d] for every row of q [R, d], fp32 on the device
    (mvlpt_op_nearest_rows; order, NaN rule and limits in include/mvlpt_hip.h)."""
    q, table = _req(q, torch.float32, "q"), _req(table, torch.float32, "table")
    (R, d), V = q.shape, table.shape[0]
    if table.shape[1] != d:
        raise ValueError("q and table must have the same width")
    with torch.cuda.device(q.device):
        nb = nearest_workspace_bytes(R, V, d, k)
        ws = torch.empty(max(nb, 8) // 8, device=q.device, dtype=torch.int64)
        idx = torch.empty(R, k, device=q.device, dtype=torch.int32)
        dist = torch.empty(R, k, device=q.device, dtype=torch.float32)
        _lib.check(lib.mvlpt_op_nearest_rows(_ptr(q), _ptr(table), R, V, d, int(k), _ptr(idx), _ptr(dist), _ptr(ws), nb, _stream()), None,
                   "op_nearest_rows")
    return idx, dist


def tpt_workspace_bytes(G: int, V: int, C_: int, e: int, k: int) -> int:
    """Scratch bytes mvlpt_op_tpt_head_fwd / _bwd need for these sizes (mvlpt_tpt_workspace_bytes)."""
    out = C.c_int64()
    _lib.check(lib.mvlpt_tpt_workspace_bytes(int(G), int(V), int(C_), int(e), int(k), C.byref(out)), None, "tpt_workspace_bytes")
    return int(out.value)


def _pitched(t: torch.Tensor, name: str) -> torch.Tensor:
    """fp32 [R, C] on the device with unit column stride and a row stride >= C: a column slice of a wider matrix passes in place (its
    row stride is the pitch the kernels take); anything else is copied once."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor: mvlpt_amd has no CPU path")
    if t.dim() != 2:
        raise ValueError(f"{name} must be a matrix")
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.float().contiguous()
    return t


def _eval_labels(labels: torch.Tensor, R: int, C_: int, name: str):
    """(tensor, MVLPT_LABEL_*, pitch) of int64 [R] labels or an fp32 [R, C] target matrix."""
    if labels.dim() == 1:
        labels = _req(labels, torch.int64, name)
        if labels.shape[0] != R:
            raise ValueError(f"{name} has {labels.shape[0]} rows, the scores {R}")
        return labels, _lib.LABEL_INT64, 0
    labels = _pitched(labels, name)
    if tuple(labels.shape) != (R, C_):
        raise ValueError(f"{name} has shape {tuple(labels.shape)}, the scores {(R, C_)}")
    return labels, _lib.LABEL_PROB_F32, labels.stride(0)


def _eval_rows(rows: Optional[torch.Tensor]):
    """(pointer, n_rows, the tensor that keeps the pointer alive) of an optional int32 row list; an empty list still passes a non-NULL
    pointer (NULL means every row)."""
    if rows is None:
        return None, 0, None
    rows = _req(rows, torch.int32, "rows")
    keep = rows if rows.numel() else torch.zeros(1, device=rows.device, dtype=torch.int32)
    return _ptr(keep), int(rows.numel()), keep


def op_eval_count(logits, labels, n_true, n_pred, n_hit, task=None, lo=None, hi=None, n_pred_r=None, n_hit_r=None, cmat=None, rows=None,
                  col_mask=None, col_seen=None) -> None:
    """One launch of the streaming class counters (mvlpt_op_eval_count), no host sync: the arg-max of every row of logits [B, C] (over
    all columns, and over the row's task range when task int32 [B] / lo / hi int32 [T] are given) is counted against its label (int64
    [B], or the arg-max of a float [B, C] row) into the caller's int64 device counters, which accumulate over calls."""
    logits = _pitched(logits, "logits")
    B, C_ = logits.shape
    labels, kind, lab_ld = _eval_labels(labels, B, C_, "labels")
    for name, t, numel in (("n_true", n_true, C_), ("n_pred", n_pred, C_), ("n_hit", n_hit, C_), ("n_pred_r", n_pred_r, C_),
                           ("n_hit_r", n_hit_r, C_), ("cmat", cmat, C_ * C_)):
        if t is not None and not (t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"{name} must be a contiguous int64 device tensor of {numel} elements")
    T = 0
    if task is not None:
        task, lo, hi = _req(task, torch.int32, "task"), _req(lo, torch.int32, "lo"), _req(hi, torch.int32, "hi")
        T = lo.numel()
        if task.numel() != B or hi.numel() != T:
            raise ValueError("task must have one entry per row, lo and hi one per task")
    if col_mask is not None:
        col_mask = _req(col_mask, torch.uint8, "col_mask")
        if col_mask.numel() != C_:
            raise ValueError("col_mask must have one entry per column")
    if col_seen is not None and not (col_seen.is_cuda and col_seen.dtype == torch.uint8 and col_seen.is_contiguous() and col_seen.numel() == C_):
        raise ValueError("col_seen must be a contiguous uint8 device tensor with one entry per column")
    rows_p, n_rows, _keep = _eval_rows(rows)
    if rows is not None and n_rows == 0:
        return
    with torch.cuda.device(logits.device):
        _lib.check(lib.mvlpt_op_eval_count(_ptr(logits), logits.stride(0), B, C_, _ptr(labels), kind, lab_ld, rows_p, n_rows, _ptr(task),
                                           _ptr(lo), _ptr(hi), T, _ptr(col_mask), _ptr(col_seen), _ptr(n_true), _ptr(n_pred), _ptr(n_hit), _ptr(n_pred_r),
                                           _ptr(n_hit_r), _ptr(cmat), _stream()), None, "op_eval_count")


def eval_workspace_bytes(N: int, C_: int) -> int:
    """Scratch bytes op_eval_rank_columns needs for at most N selected rows and C columns on the current stream."""
    out = C.c_int64()
    _lib.check(lib.mvlpt_eval_workspace_bytes(int(N), int(C_), _stream(), C.byref(out)), None, "eval_workspace_bytes")
    return int(out.value)


def op_eval_rank_columns(scores, targets, rows=None, thresholds=None) -> Dict[str, torch.Tensor]:
    """Sorted-order statistics of every column of scores [N, C] over the rows of the optional int32 list `rows` (None: all; may be
    empty) against int64 [N] labels or a float [N, C] target matrix (mvlpt_op_eval_rank_columns): device tensors n_pos / n_neg /
    twice_u int64 [C], interp float64 [C, 11], flags int32 [C], all views of the one int64 buffer "packed" (one copy reads them back:
    `unpack_eval_rank`).  A column slice is read in place."""
    scores = _pitched(scores, "scores")
    N, C_ = scores.shape
    targets, kind, tgt_ld = _eval_labels(targets, N, C_, "targets")
    if thresholds is None:
        import numpy as np
        thresholds = np.linspace(1, 0, _lib.EVAL_POINTS, endpoint=True).tolist()
    if len(thresholds) != _lib.EVAL_POINTS:
        raise ValueError(f"{_lib.EVAL_POINTS} thresholds are needed")
    th = (C.c_double * _lib.EVAL_POINTS)(*thresholds)
    rows_p, n_rows, _keep = _eval_rows(rows)
    P = _lib.EVAL_POINTS
    with torch.cuda.device(scores.device):
        packed = torch.zeros(C_ * (3 + P) + (C_ + 1) // 2, device=scores.device, dtype=torch.int64)      # (the odd flag word is padding)
        out = unpack_eval_rank(packed, C_)
        nb = eval_workspace_bytes(N if rows is None else max(n_rows, 1), C_)
        ws = torch.empty(nb // 8, device=scores.device, dtype=torch.int64) if nb else None
        _lib.check(lib.mvlpt_op_eval_rank_columns(_ptr(scores), scores.stride(0), N, C_, _ptr(targets), kind, tgt_ld, rows_p, n_rows, th,
                                                  _ptr(out["n_pos"]), _ptr(out["n_neg"]), _ptr(out["twice_u"]), _ptr(out["interp"]),
                                                  _ptr(out["flags"]), _ptr(ws), nb, _stream()), None, "op_eval_rank_columns")
    out["packed"] = packed
    return out


def unpack_eval_rank(packed, C_: int):
    """The five arrays of op_eval_rank_columns as views of its packed int64 buffer (a torch tensor on any device)."""
    P = _lib.EVAL_POINTS
    return {"n_pos": packed[:C_], "n_neg": packed[C_:2 * C_], "twice_u": packed[2 * C_:3 * C_],
            "interp": packed[3 * C_:(3 + P) * C_].view(torch.float64).view(C_, P),
            "flags": packed[(3 + P) * C_:].view(torch.int32)[:C_]}


def softmax_reg_workspace_bytes(N: int, D: int, K: int) -> int:
    """Scratch bytes op_softmax_reg_eval / op_softmax_reg_predict need for these sizes (mvlpt_softmax_reg_workspace_bytes)."""
    out = C.c_size_t()
    _lib.check(lib.mvlpt_softmax_reg_workspace_bytes(int(N), int(D), int(K), C.byref(out)), None, "softmax_reg_workspace_bytes")
    return int(out.value)


def softmax_reg_workspace(N: int, D: int, K: int, device) -> torch.Tensor:
    """A workspace of softmax_reg_workspace_bytes for these sizes (int64 elements: 8-byte units of an aligned allocation)."""
    return torch.empty((softmax_reg_workspace_bytes(N, D, K) + 7) // 8, device=device, dtype=torch.int64)


def op_softmax_reg_eval(X, y, theta, l2: float, dir=None, grad=None, stats=None, ws=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad fp32 [K*D + K], stats float64 [4] = F, max|grad|, grad . dir, |grad|^2) of the softmax-regression objective at
    theta = [W [K, D] | b [K]] for X fp32 [N, D] and labels y int32 [N] in [0, K), all on the device (mvlpt_op_softmax_reg_eval;
    arithmetic and limits in include/mvlpt_hip.h).  Enqueue-only: nothing is read back.  grad / stats / ws may be passed to reuse
    buffers over the evaluations of a fit."""
    X, y, theta = _req(X, torch.float32, "X"), _req(y, torch.int32, "y"), _req(theta, torch.float32, "theta")
    N, D = X.shape
    if y.shape != (N,):
        raise ValueError("y must hold one label per row of X")
    if theta.dim() != 1 or theta.numel() % (D + 1):
        raise ValueError("theta must be flat with K * D + K elements")
    K = theta.numel() // (D + 1)
    if dir is not None:
        dir = _req(dir, torch.float32, "dir")
        if dir.shape != theta.shape:
            raise ValueError("dir must have theta's shape")
    with torch.cuda.device(X.device):
        ws = softmax_reg_workspace(N, D, K, X.device) if ws is None else ws
        grad = torch.empty_like(theta) if grad is None else _req(grad, torch.float32, "grad")
        stats = torch.empty(4, device=X.device, dtype=torch.float64) if stats is None else _req(stats, torch.float64, "stats")
        if grad.numel() < theta.numel() or stats.numel() < 4:
            raise ValueError("grad / stats are too small")
        _lib.check(lib.mvlpt_op_softmax_reg_eval(_ptr(X), _ptr(y), _ptr(theta), _ptr(dir), N, D, K, float(l2), _ptr(grad), _ptr(stats),
                                                 _ptr(ws), ws.numel() * ws.element_size(), _stream()), None, "op_softmax_reg_eval")
    return grad, stats


def op_softmax_reg_predict(X, theta, margin: bool = False, ws=None):
    """pred int32 [N] (and margin fp32 [N] = largest - second largest logit when asked) of theta = [W [K, D] | b [K]] on X fp32 [N, D]
    (mvlpt_op_softmax_reg_predict: equal logits go to the lowest class index)."""
    X, theta = _req(X, torch.float32, "X"), _req(theta, torch.float32, "theta")
    N, D = X.shape
    if theta.dim() != 1 or theta.numel() % (D + 1):
        raise ValueError("theta must be flat with K * D + K elements")
    K = theta.numel() // (D + 1)
    with torch.cuda.device(X.device):
        ws = softmax_reg_workspace(N, D, K, X.device) if ws is None else ws
        pred = torch.empty(N, device=X.device, dtype=torch.int32)
        mg = torch.empty(N, device=X.device, dtype=torch.float32) if margin else None
        _lib.check(lib.mvlpt_op_softmax_reg_predict(_ptr(X), _ptr(theta), N, D, K, _ptr(pred), _ptr(mg), _ptr(ws),
                                                    ws.numel() * ws.element_size(), _stream()), None, "op_softmax_reg_predict")
    return (pred, mg) if margin else pred


def op_ensemble_features(feats) -> torch.Tensor:
    feats = _req(feats, torch.float32, "feats")
    T, Cn, e = feats.shape
    out = torch.empty(Cn, e, device=feats.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_ensemble_features(_ptr(feats), _ptr(out), T, Cn, e, _stream()), None, "op_ensemble_features")
    return out


def op_normalize_rows(x):
    """(x / |x|, |x|) per row: the head's normalisation kernel."""
    x = _req(x, torch.float32, "x")
    rows, d = x.shape
    xn, norm = torch.empty_like(x), torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_normalize_rows(_ptr(x), _ptr(xn), _ptr(norm), rows, d, _stream()), None, "op_normalize_rows")
    return xn, norm


def op_sgemm_bt(A, Bt, alpha=None) -> torch.Tensor:
    """fp32 C [M, N] = alpha * A [M, K] @ Bt [N, K]^T (mvlpt_op_sgemm_bt); alpha: a device float tensor or None."""
    M, K = A.shape
    N = Bt.shape[0]
    out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_sgemm_bt(_ptr(A.contiguous()), _ptr(Bt.contiguous()), _ptr(out), M, N, K, _ptr(alpha), _stream()), None,
               "op_sgemm_bt")
    return out


def op_grad_scale(v: torch.Tensor, target: float) -> torch.Tensor:
    """scale_dev = {2^k, 2^-k, amax|v|} (3 floats on the device) of the flat fp32 tensor `v`, which is read where it lies: a view that
    starts 4 bytes into an allocation takes the two-stage path at any length."""
    if v.dim() != 1 or v.stride(0) != 1 or v.dtype != torch.float32:
        raise ValueError("op_grad_scale wants a flat fp32 tensor with unit stride")
    sc = torch.full((3,), float("nan"), device=v.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_grad_scale(_ptr(v), v.numel(), float(target), _ptr(sc), _stream()), None, "op_grad_scale")
    return sc


def op_reduce_prompt_rows(dx32, dx16, row0: int, n: int, scale_dev=None, zero_after=False, split16=0, vmask=None) -> torch.Tensor:
    """out [n, d] = scale_dev[1] * sum_b dx32[b, row0 + j] (* vmask[b, j]); dx32 [B, L, d] (and its 16-bit copy dx16 [B * L, d or 2d], or
    None) are cleared IN PLACE at those rows when zero_after."""
    B, L, d = dx32.shape
    if not dx32.is_contiguous() or (dx16 is not None and not dx16.is_contiguous()):
        raise ValueError("op_reduce_prompt_rows works in place: contiguous tensors only")
    dt = _TORCH2DT[dx16.dtype] if dx16 is not None else DT_F16
    out = torch.empty(n, d, device=dx32.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_reduce_prompt_rows(dt, _ptr(dx32), _ptr(dx16), B, L, d, row0, n, _ptr(out), _ptr(scale_dev), int(zero_after),
                                               int(split16), _ptr(vmask), _stream()), None, "op_reduce_prompt_rows")
    return out


def op_gather_ctx_grad(dx, ctx_pos, per_class: bool, scale_dev=None) -> torch.Tensor:
    """dctx [n, d] (generic: summed over the classes) or [C, n, d] (per class) from dx [C, L, d] at ctx_pos [C, n]."""
    C_, L, d = dx.shape
    n = ctx_pos.shape[1]
    dctx = torch.empty((C_, n, d) if per_class else (n, d), device=dx.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_gather_ctx_grad(_ptr(dx.contiguous()), _ptr(ctx_pos.to(torch.int32).contiguous()), C_, L, d, n, int(per_class),
                                            _ptr(dctx), _ptr(scale_dev), _stream()), None, "op_gather_ctx_grad")
    return dctx


def op_attention_bwd_cls(qkv, o_cls, do_cls, lse, N, L, H, fill=float("nan")) -> torch.Tensor:
    """dqkv [N*L, 3*H*64] of the CLS-only attention backward; the output is pre-filled with `fill` (the kernel writes every element)."""
    dqkv = torch.full_like(qkv, fill)
    _lib.check(lib.mvlpt_op_attention_bwd_cls(_TORCH2DT[qkv.dtype], _ptr(qkv.contiguous()), _ptr(o_cls.contiguous()),
                                              _ptr(do_cls.contiguous()), _ptr(lse.contiguous()), _ptr(dqkv), N, L, H, _stream()), None,
               "op_attention_bwd_cls")
    return dqkv


def op_copy_rows(src, idx, dst=None) -> torch.Tensor:
    """Gather (dst is None): returns src[idx].  Scatter: dst[idx[r]] = src[r] IN PLACE on the contiguous `dst`, which is returned."""
    idx = idx.to(torch.int32).contiguous()
    src = src.contiguous()
    row_bytes = src[0].numel() * src.element_size()
    scatter = dst is not None
    if scatter and not dst.is_contiguous():
        raise ValueError("op_copy_rows scatters in place: contiguous dst only")
    if not scatter:
        dst = torch.empty((idx.numel(),) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype)
    _lib.check(lib.mvlpt_op_copy_rows(_ptr(src), _ptr(dst), _ptr(idx), idx.numel(), row_bytes, int(scatter), _stream()), None, "op_copy_rows")
    return dst


def op_overwrite_rows(rows, x, vmask=None) -> torch.Tensor:
    """x[b, 1 + j] = rows[j] (* vmask[b, j]) IN PLACE on the contiguous x [B, L, d], which is returned."""
    B, L, d = x.shape
    if not x.is_contiguous():
        raise ValueError("op_overwrite_rows works in place: contiguous x only")
    _lib.check(lib.mvlpt_op_overwrite_rows(_ptr(rows.contiguous()), rows.shape[0], _ptr(x), B, L, d, _ptr(vmask), _stream()), None,
               "op_overwrite_rows")
    return x


def op_overwrite_ctx_rows(rows, ctx_pos, x) -> torch.Tensor:
    """x[c, ctx_pos[c, j]] = rows[j] IN PLACE on the contiguous fp32 x [C, L, d], which is returned; ctx_pos int32 [C, n_ctx]."""
    C_, L, d = x.shape
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise ValueError("op_overwrite_ctx_rows works in place: contiguous fp32 x only")
    _lib.check(lib.mvlpt_op_overwrite_ctx_rows(_ptr(rows.contiguous()), _ptr(ctx_pos.to(torch.int32).contiguous()), _ptr(x), C_, L, d,
                                               ctx_pos.shape[1], _stream()), None, "op_overwrite_ctx_rows")
    return x


def op_gather_zero_ctx_grad(dx32, dx16, ctx_pos, split16=0, scale_dev=None, dtype=None) -> torch.Tensor:
    """out [n_ctx, d] = scale_dev[1] * sum_c dx32[c, ctx_pos[c, j]]; those rows of dx32 [C, L, d] and of its 16-bit copy dx16
    ([C * L, d or 2d], or None) are zeroed IN PLACE."""
    C_, L, d = dx32.shape
    if not dx32.is_contiguous() or dx32.dtype != torch.float32 or (dx16 is not None and not dx16.is_contiguous()):
        raise ValueError("op_gather_zero_ctx_grad works in place: contiguous tensors only")
    dt = _TORCH2DT[dx16.dtype] if dx16 is not None else (_TORCH2DT[dtype] if dtype is not None else DT_F16)
    n = ctx_pos.shape[1]
    out = torch.empty(n, d, device=dx32.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_gather_zero_ctx_grad(dt, _ptr(dx32), _ptr(dx16), int(split16), _ptr(ctx_pos.to(torch.int32).contiguous()), C_, L,
                                                 d, n, _ptr(out), _ptr(scale_dev), _stream()), None, "op_gather_zero_ctx_grad")
    return out


def op_assemble_tokens(pe, cls, pos, g, b, batch: int, vpt=None, vmask=None, fill=float("nan")) -> torch.Tensor:
    """x [batch, 1 + n_vpt + G2, d] of the image tower's entry from pe [batch * G2, d], cls [d], pos [1 + G2, d], ln_pre (g, b),
    vpt [n_vpt, d] or None and its dropout mask [batch, n_vpt, d] or None; pre-filled with `fill`."""
    d = pe.shape[1]
    G2 = pe.shape[0] // batch
    n_vpt = 0 if vpt is None else vpt.shape[0]
    x = torch.full((batch, 1 + n_vpt + G2, d), fill, device=pe.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_assemble_tokens(_ptr(pe.contiguous()), _ptr(cls.contiguous()), _ptr(pos.contiguous()), _ptr(g.contiguous()),
                                            _ptr(b.contiguous()), _ptr(None if vpt is None else vpt.contiguous()), n_vpt,
                                            _ptr(None if vmask is None else vmask.contiguous()), _ptr(x), batch, G2, d, _stream()),
               None, "op_assemble_tokens")
    return x


def op_assemble_prompts(prefix, suffix, ctx, layout, pos, eot):
    """(x [C, L, d], ctx_pos int32 [C, n] or None, eot_rows int32 [C]) of the text tower's entry: ctx [n, d] (generic), [C, n, d] (per
    class) or None (n = 0)."""
    C_, L = layout.shape
    d = prefix.shape[-1]
    n = 0 if ctx is None else ctx.shape[-2]
    x = torch.full((C_, L, d), float("nan"), device=prefix.device, dtype=torch.float32)
    ctx_pos = torch.full((C_, n), -1, device=prefix.device, dtype=torch.int32) if n else None
    rows = torch.full((C_,), -1, device=prefix.device, dtype=torch.int32)
    _lib.check(lib.mvlpt_op_assemble_prompts(_ptr(prefix.contiguous()), _ptr(suffix.contiguous()),
                                             _ptr(None if ctx is None else ctx.contiguous()), int(ctx is not None and ctx.dim() == 3), n,
                                             _ptr(layout.to(torch.int32).contiguous()), _ptr(pos.contiguous()),
                                             _ptr(eot.to(torch.int32).contiguous()), _ptr(x), _ptr(ctx_pos), _ptr(rows), C_, L, d,
                                             _stream()), None, "op_assemble_prompts")
    return x, ctx_pos, rows


def op_cast_mixed(x32: torch.Tensor, dtype) -> torch.Tensor:
    rows, d = x32.shape
    out = torch.zeros(rows, 2 * d, device=x32.device, dtype=dtype)
    _lib.check(lib.mvlpt_op_cast_mixed(_TORCH2DT[dtype], _ptr(x32.contiguous()), _ptr(out), rows, d, _stream()), None, "op_cast_mixed")
    return out


def op_pack_weight_mixed(w32: torch.Tensor, dtype, transposed=False):
    """nn.Linear weight [out, in] fp32 -> (packed [R, 3K/2] 16-bit elements = [W16 | e4m3(W * 2^e8) bytes], e8)."""
    rows, cols = w32.shape
    R, K = (cols, rows) if transposed else (rows, cols)
    out = torch.zeros(R, K + K // 2, device=w32.device, dtype=dtype)
    e8 = C.c_int(0)
    _lib.check(lib.mvlpt_op_pack_weight_mixed(_TORCH2DT[dtype], _ptr(w32.contiguous()), rows, cols, int(transposed), _ptr(out),
                                              C.byref(e8), _stream()), None, "op_pack_weight_mixed")
    return out, e8.value


def op_gemm_mixed(A2, Wp, e8, epi=_lib.EPI_STORE32, bias=None, aux=None, resid=None, out2=False):
    """A2: mixed pair [M, 2K]; Wp: packed weight [N, 3K/2] from op_pack_weight_mixed."""
    dt = _TORCH2DT[A2.dtype]
    M, K = A2.shape[0], A2.shape[1] // 2
    N = Wp.shape[0]
    if epi in (_lib.EPI_RESID32, _lib.EPI_STORE32):
        out = torch.empty(M, N, device=A2.device, dtype=torch.float32)
    else:
        out = torch.zeros(M, 2 * N, device=A2.device, dtype=A2.dtype)
    o2 = torch.empty(M, N, device=A2.device, dtype=A2.dtype) if out2 else None
    _lib.check(lib.mvlpt_op_gemm_mixed(dt, epi, _ptr(A2.contiguous()), _ptr(Wp), Wp.shape[1], e8, M, N, K, _ptr(bias), _ptr(aux),
                                       _ptr(resid), _ptr(out), _ptr(o2), _stream()), None, "op_gemm_mixed")
    return (out, o2) if out2 else out


def op_layernorm_fwd_mixed(x, gamma, beta, out_dtype):
    rows, d = x.shape
    y = torch.zeros(rows, 2 * d, device=x.device, dtype=out_dtype)
    _lib.check(lib.mvlpt_op_layernorm_fwd_mixed(_TORCH2DT[out_dtype], _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), rows, d, _stream()),
               None, "op_layernorm_fwd_mixed")
    return y


def op_layernorm_bwd_mixed(dy32, x, gamma, dtype, resid=None):
    rows, d = x.shape
    out32 = torch.empty(rows, d, device=x.device, dtype=torch.float32)
    out16 = torch.zeros(rows, 2 * d, device=x.device, dtype=dtype)
    _lib.check(lib.mvlpt_op_layernorm_bwd_mixed(_TORCH2DT[dtype], _ptr(dy32), _ptr(x), _ptr(gamma), _ptr(resid), _ptr(out32),
                                                _ptr(out16), rows, d, _stream()), None, "op_layernorm_bwd_mixed")
    return out32, out16


def op_attention32_fwd_mixed(qkv_pair, N, L, H, causal, q_rows=0):
    """qkv: 16-bit pair [N*L, 6d] -> (O as a mixed pair [N*L, 2d], lse)."""
    dtype = qkv_pair.dtype
    out = torch.zeros(N * L, 2 * H * 64, device=qkv_pair.device, dtype=dtype)
    lse = torch.zeros(N * H * L, device=qkv_pair.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_attention32_fwd_mixed(_TORCH2DT[dtype], _ptr(qkv_pair), _ptr(out), _ptr(lse), N, L, H, int(causal), q_rows,
                                                  _stream()), None, "op_attention32_fwd_mixed")
    return out, lse


def op_attention32_bwd_mixed(qkv_pair, out_mixed, dout_pair, lse, N, L, H, causal):
    """-> dqkv as a mixed pair [N*L, 6d] (hi plane 3d wide)."""
    dtype = out_mixed.dtype
    dqkv = torch.zeros(N * L, 6 * H * 64, device=qkv_pair.device, dtype=dtype)
    delta = torch.empty(N * H * L, device=qkv_pair.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_attention32_bwd_mixed(_TORCH2DT[dtype], _ptr(qkv_pair), _ptr(out_mixed), _ptr(dout_pair), _ptr(lse),
                                                  _ptr(delta), _ptr(dqkv), N, L, H, int(causal), _stream()), None, "op_attention32_bwd_mixed")
    return dqkv


def op_layernorm_fwd_split(x, gamma, beta, out_dtype):
    rows, d = x.shape
    y = torch.empty(rows, 2 * d, device=x.device, dtype=out_dtype)
    _lib.check(lib.mvlpt_op_layernorm_fwd_split(_TORCH2DT[out_dtype], _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), rows, d, _stream()),
               None, "op_layernorm_fwd_split")
    return y


def op_layernorm_bwd_split(dy32, x, gamma, dtype, resid=None):
    rows, d = x.shape
    out32 = torch.empty(rows, d, device=x.device, dtype=torch.float32)
    out16 = torch.empty(rows, 2 * d, device=x.device, dtype=dtype)
    _lib.check(lib.mvlpt_op_layernorm_bwd_split(_TORCH2DT[dtype], _ptr(dy32), _ptr(x), _ptr(gamma), _ptr(resid), _ptr(out32),
                                                _ptr(out16), rows, d, _stream()), None, "op_layernorm_bwd_split")
    return out32, out16


def op_attention32_fwd_pair(qkv_pair, N, L, H, causal, q_rows=0):
    """Split-precision attention core: qkv hi|lo pair [N*L, 6d] -> (O pair [N*L, 2d], lse)."""
    dtype = qkv_pair.dtype
    out = torch.zeros(N * L, 2 * H * 64, device=qkv_pair.device, dtype=dtype)
    lse = torch.zeros(N * H * L, device=qkv_pair.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_attention32_fwd(_TORCH2DT[dtype], _ptr(qkv_pair), _ptr(out), _ptr(lse), N, L, H, int(causal), q_rows,
                                            _stream()), None, "op_attention32_fwd")
    return out, lse


def op_attention32_bwd_pair(qkv_pair, out_pair, dout_pair, lse, N, L, H, causal):
    dtype = out_pair.dtype
    dqkv = torch.empty(N * L, 6 * H * 64, device=qkv_pair.device, dtype=dtype)
    delta = torch.empty(N * H * L, device=qkv_pair.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_attention32_bwd(_TORCH2DT[dtype], _ptr(qkv_pair), _ptr(out_pair), _ptr(dout_pair), _ptr(lse),
                                            _ptr(delta), _ptr(dqkv), N, L, H, int(causal), _stream()), None, "op_attention32_bwd")
    return dqkv


def op_attention32_fwd(qkv32, N, L, H, causal, dtype=torch.float16, q_rows=0):
    """Same on fp32 inputs, split to pairs here (as the QKV GEMM's epilogue does in the engine)."""
    return op_attention32_fwd_pair(split_pair(qkv32, dtype), N, L, H, causal, q_rows)


def op_attention32_bwd(qkv32, out_pair, dout32, lse, N, L, H, causal):
    dtype = out_pair.dtype
    return op_attention32_bwd_pair(split_pair(qkv32, dtype), out_pair, split_pair(dout32, dtype), lse, N, L, H, causal)


def op_layernorm_fwd(x, gamma, beta, out_dtype):
    rows, d = x.shape
    y = torch.empty(rows, d, device=x.device, dtype=out_dtype)
    _lib.check(lib.mvlpt_op_layernorm_fwd(_TORCH2DT[out_dtype], _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), rows, d, _stream()),
               None, "op_layernorm_fwd")
    return y


def op_layernorm_bwd(dy, x, gamma, resid=None, want16=True):
    rows, d = x.shape
    out32 = torch.empty(rows, d, device=x.device, dtype=torch.float32)
    out16 = torch.empty(rows, d, device=x.device, dtype=dy.dtype) if want16 else None
    _lib.check(lib.mvlpt_op_layernorm_bwd(_TORCH2DT[dy.dtype], _ptr(dy), _ptr(x), _ptr(gamma), _ptr(resid), _ptr(out32),
                                          _ptr(out16), rows, d, _stream()), None, "op_layernorm_bwd")
    return out32, out16


def _dt(dtype) -> int:
    """A torch dtype, or the raw MVLPT_DT_* integer (refusal tests pass unknown ones)."""
    return dtype if isinstance(dtype, int) else _TORCH2DT[dtype]


def op_layernorm_fwd_ex(x, gamma, beta, y, rows, d, row_mul=1, split=0, out_dtype=None):
    """mvlpt_op_layernorm_fwd_ex on caller-owned tensors (nothing is copied, allocated or made contiguous)."""
    _lib.check(lib.mvlpt_op_layernorm_fwd_ex(_dt(y.dtype if out_dtype is None else out_dtype), _ptr(x), row_mul, _ptr(gamma), _ptr(beta),
                                             _ptr(y), rows, d, split, _stream()), None, "op_layernorm_fwd_ex")
    return y


def op_layernorm_bwd_ex(dy, x, gamma, out32, rows, d, dtype, resid=None, out16=None, row_mul=1, split=0, dy_dtype=None):
    """mvlpt_op_layernorm_bwd_ex on caller-owned tensors; out32 may be `resid` itself."""
    _lib.check(lib.mvlpt_op_layernorm_bwd_ex(_dt(dtype), _ptr(dy), _dt(dy.dtype if dy_dtype is None else dy_dtype), _ptr(x), row_mul,
                                             _ptr(gamma), _ptr(resid), _ptr(out32), _ptr(out16), rows, d, split, _stream()),
               None, "op_layernorm_bwd_ex")
    return out32, out16


def op_layernorm_route(rows, d):
    """(0 direct / 1 grid-stride, float4 per lane of the instantiation, workgroups) of a LayerNorm launch on the current stream."""
    nv, grid = C.c_int(0), C.c_int(0)
    kind = lib.mvlpt_op_layernorm_route(rows, d, _stream(), C.byref(nv), C.byref(grid))
    if kind < 0:
        raise RuntimeError(f"libmvlpt_hip op_layernorm_route failed (code {kind}): {_lib.last_error(None)}")
    return kind, nv.value, grid.value


def op_cast_ex(x32, out, rows, d, fmt=0, scale_dev=None, dtype=None):
    """mvlpt_op_cast_ex: fmt 0 plain, 1 hi|lo pair, 2 mixed pair; scale_dev a device float tensor or None."""
    _lib.check(lib.mvlpt_op_cast_ex(_dt(out.dtype if dtype is None else dtype), _ptr(x32), _ptr(out), rows, d, fmt, _ptr(scale_dev),
                                    _stream()), None, "op_cast_ex")
    return out


def op_cast_to_f32(x, out, n, in_dtype=None):
    _lib.check(lib.mvlpt_op_cast_to_f32(_dt(x.dtype if in_dtype is None else in_dtype), _ptr(x), _ptr(out), n, _stream()), None,
               "op_cast_to_f32")
    return out


def op_pack_weight(w32, out, rows, cols, transposed=False, ld_out=0, dtype=None):
    _lib.check(lib.mvlpt_op_pack_weight(_dt(out.dtype if dtype is None else dtype), _ptr(w32), rows, cols, int(transposed), ld_out,
                                        _ptr(out), _stream()), None, "op_pack_weight")
    return out


def op_patchify(image, out, B, R, P, Kp, dtype=None, image_dtype=None):
    _lib.check(lib.mvlpt_op_patchify(_dt(out.dtype if dtype is None else dtype), _ptr(image),
                                     _dt(image.dtype if image_dtype is None else image_dtype), _ptr(out), B, R, P, Kp, _stream()),
               None, "op_patchify")
    return out


def op_patchify_route(dtype, image_dtype, R, P):
    """0 scalar, 1 vector, 2 the 16-byte copy: the kernel op_patchify uses."""
    route = lib.mvlpt_op_patchify_route(_dt(dtype), _dt(image_dtype), R, P)
    if route < 0:
        raise RuntimeError(f"libmvlpt_hip op_patchify_route failed (code {route}): {_lib.last_error(None)}")
    return route


def op_attention_fwd(qkv, N, L, H, causal, want_lse=True):
    out = torch.empty(N * L, H * 64, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(N * H * L, device=qkv.device, dtype=torch.float32) if want_lse else None
    _lib.check(lib.mvlpt_op_attention_fwd(_TORCH2DT[qkv.dtype], _ptr(qkv), _ptr(out), _ptr(lse), N, L, H, int(causal), _stream()),
               None, "op_attention_fwd")
    return out, lse


def op_attention_wide_fwd(qkv, N, L, H, head_width, q_rows=0, want_lse=True, out=None, lse=None):
    """The forward for heads wider than 64 (mvlpt_op_attention_wide_fwd): qkv [N*L, 3*H*w] -> (out [N*L, H*w], lse [N*H*L] or None).
    out / lse: caller-owned destinations (contiguous views; q_rows > 0 writes only rows 0..q_rows-1 of every sequence)."""
    if out is None:
        out = torch.empty(N * L, H * head_width, device=qkv.device, dtype=qkv.dtype)
    if lse is None and want_lse:
        lse = torch.empty(N * H * L, device=qkv.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_attention_wide_fwd(_TORCH2DT[qkv.dtype], _ptr(qkv), _ptr(out), _ptr(lse), N, L, H, int(head_width), int(q_rows),
                                               _stream()), None, "op_attention_wide_fwd")
    return out, lse


def op_attention_bwd(qkv, out, dout, lse, N, L, H, causal):
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(N * H * L, device=qkv.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_attention_bwd(_TORCH2DT[qkv.dtype], _ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(delta),
                                          _ptr(dqkv), N, L, H, int(causal), _stream()), None, "op_attention_bwd")
    return dqkv


# ---- LayerNorm folding at kernel level (include/mvlpt_hip.h: mvlpt_op_fold_vectors / gemm_ln_producer / gemm_folded)
def op_fold_vectors(W16: torch.Tensor, K: int, gamma, beta, b):
    """W16: packed 16-bit weight [N, ld >= K] -> (colsum = W gamma, bias2 = b + W beta), fp32 [N]."""
    N, ld = W16.shape
    cs = torch.empty(N, device=W16.device, dtype=torch.float32)
    b2 = torch.empty(N, device=W16.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_fold_vectors(_TORCH2DT[W16.dtype], _ptr(W16), ld, _ptr(gamma), _ptr(beta), _ptr(b), _ptr(cs), _ptr(b2), N, K,
                                         _stream()), None, "op_fold_vectors")
    return cs, b2


def op_gemm_ln_producer(A, Bt, bias, resid, gamma, a_split=0, x16_split=0, ldb=0, w8_exp=0, ntp=8):
    """-> (out32 [M,N], x16 (format x16_split), part [M, ntp, 2], nt)."""
    dtype = A.dtype
    M = A.shape[0]
    K = A.shape[1] // (2 if a_split else 1)
    N = Bt.shape[0]
    out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    x16 = torch.zeros(M, N * (2 if x16_split else 1), device=A.device, dtype=dtype)
    part = torch.zeros(M, ntp, 2, device=A.device, dtype=torch.float32)
    nt = C.c_int(0)
    _lib.check(lib.mvlpt_op_gemm_ln_producer(_TORCH2DT[dtype], _ptr(A.contiguous()), a_split, _ptr(Bt), ldb, w8_exp, M, N, K, _ptr(bias),
                                             _ptr(resid), _ptr(gamma), x16_split, _ptr(out), _ptr(x16), _ptr(part), ntp, C.byref(nt),
                                             _stream()), None, "op_gemm_ln_producer")
    return out, x16, part, nt.value


# ---- packed residual stream at kernel level (include/mvlpt_hip.h: mvlpt_op_fold_weight / respk_pack / respk_unpack / gemm_residp)
def op_fold_weight(W16: torch.Tensor, K: int, gamma):
    """W16 fp16 [N, ld >= K] -> (Wg = round16(W16 * gamma) [N, K], colsum = row sums of Wg, fp32 [N])."""
    N, ld = W16.shape
    Wg = torch.empty(N, K, device=W16.device, dtype=torch.float16)
    cs = torch.empty(N, device=W16.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_fold_weight(_ptr(W16), ld, _ptr(gamma), _ptr(Wg), K, _ptr(cs), N, K, _stream()), None, "op_fold_weight")
    return Wg, cs


def op_respk_pack(x: torch.Tensor, ntp: int = 0):
    """fp32 [rows, d] -> (hi fp16 [rows, d], lo int8 [rows, d], part [rows, ntp, 2] or None)."""
    rows, d = x.shape
    hi = torch.empty(rows, d, device=x.device, dtype=torch.float16)
    lo = torch.empty(rows, d, device=x.device, dtype=torch.int8)
    part = torch.full((rows, ntp, 2), float("nan"), device=x.device, dtype=torch.float32) if ntp else None
    _lib.check(lib.mvlpt_op_respk_pack(_ptr(x.contiguous()), _ptr(hi), _ptr(lo), _ptr(part), ntp, rows, d, _stream()), None, "op_respk_pack")
    return hi, lo, part


def op_assemble_packed(pe: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, g: torch.Tensor, b: torch.Tensor, batch: int, ntp: int = 6):
    """patch embeddings fp32 [batch * G2, d] -> the packed tower entry: (hi fp16 [batch * (1 + G2), d], lo int8, part [rows, ntp, 2])."""
    d = pe.shape[1]
    G2 = pe.shape[0] // batch
    rows = batch * (1 + G2)
    hi = torch.empty(rows, d, device=pe.device, dtype=torch.float16)
    lo = torch.empty(rows, d, device=pe.device, dtype=torch.int8)
    part = torch.empty(rows, ntp, 2, device=pe.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_assemble_packed(_ptr(pe), _ptr(cls), _ptr(pos), _ptr(g), _ptr(b), _ptr(hi), _ptr(lo), _ptr(part), ntp, batch, G2, d,
                                            _stream()), None, "op_assemble_packed")
    return hi, lo, part


def op_respk_unpack(hi: torch.Tensor, lo: torch.Tensor, row_mul: int = 1):
    rows, d = hi.shape[0] // row_mul, hi.shape[1]
    out = torch.empty(rows, d, device=hi.device, dtype=torch.float32)
    _lib.check(lib.mvlpt_op_respk_unpack(_ptr(hi), _ptr(lo), row_mul, _ptr(out), rows, d, _stream()), None, "op_respk_unpack")
    return out


def op_gemm_residp(A, Bt, bias, hi, lo, ldb=0, ntp=8, in_place=False):
    """(hi', lo') = pack(A Bt^T + bias + unpack(hi, lo)); -> (hi', lo', part [M, ntp, 2], nt)."""
    M, K = A.shape
    N = Bt.shape[0]
    ho = hi if in_place else torch.empty_like(hi)
    lo_o = lo if in_place else torch.empty_like(lo)
    part = torch.zeros(M, ntp, 2, device=A.device, dtype=torch.float32)
    nt = C.c_int(0)
    _lib.check(lib.mvlpt_op_gemm_residp(_ptr(A.contiguous()), _ptr(Bt), ldb, M, N, K, _ptr(bias), _ptr(hi), _ptr(lo), _ptr(ho), _ptr(lo_o),
                                        _ptr(part), ntp, C.byref(nt), _stream()), None, "op_gemm_residp")
    return ho, lo_o, part, nt.value


def op_gemm_folded(x16, Bt, colsum, bias2, part, nt, epi=_lib.EPI_STORE16, a_split=0, ldb=0, w8_exp=0, out2=False):
    dtype = x16.dtype
    M = x16.shape[0]
    K = x16.shape[1] // (2 if a_split else 1)
    N = Bt.shape[0]
    wide = epi in (_lib.EPI_GELU_SPLIT, _lib.EPI_STORE_SPLIT)
    out = torch.zeros(M, N * (2 if wide else 1), device=x16.device, dtype=dtype)
    o2 = torch.empty(M, N, device=x16.device, dtype=dtype) if out2 else None
    _lib.check(lib.mvlpt_op_gemm_folded(_TORCH2DT[dtype], epi, _ptr(x16), a_split, _ptr(Bt), ldb, w8_exp, M, N, K, _ptr(colsum), _ptr(bias2),
                                        _ptr(part), part.shape[1], nt, _ptr(out), _ptr(o2), _stream()), None, "op_gemm_folded")
    return (out, o2) if out2 else out


# ------------------------------------------------------------------------------------------------ convolutional tower at kernel level
def conv_out_size(n: int, k: int, stride: int) -> int:
    return (n + 2 * (k // 2) - k) // stride + 1


def op_pack_conv_weight(w32: torch.Tensor, cin_pad: Optional[int] = None) -> torch.Tensor:
    """w32 [Cout, Cin, k, k] fp32 -> the packed fp16 [Cout, Kp] weight of mvlpt_op_conv2d (tap-major, zero padded)."""
    w32 = _req(w32, torch.float32, "w32")
    cout, cin, k, _ = w32.shape
    cin_pad = cin_pad or (cin + 7) // 8 * 8
    kp = C.c_int(0)
    _lib.check(lib.mvlpt_op_pack_conv_weight(None, cout, cin, k, cin_pad, None, C.byref(kp), _stream()), None, "op_pack_conv_weight")
    out = torch.empty(cout, kp.value, device=w32.device, dtype=torch.float16)
    _lib.check(lib.mvlpt_op_pack_conv_weight(_ptr(w32), cout, cin, k, cin_pad, _ptr(out), None, _stream()), None, "op_pack_conv_weight")
    return out


def op_conv2d_raw(x, w, scale, shift, resid, y, B, H, W, Cin, Cout, k, stride, relu) -> int:
    """mvlpt_op_conv2d with nothing checked on this side: returns the library's code."""
    return lib.mvlpt_op_conv2d(_ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(resid), _ptr(y), B, H, W, Cin, Cout, k, stride,
                               int(relu), _stream())


def op_conv2d(x: torch.Tensor, w_packed: torch.Tensor, scale, shift, k: int, stride: int = 1, relu: bool = False, resid=None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B, H, W, Cin] fp16 NHWC -> [B, Ho, Wo, Cout] fp16 (include/mvlpt_hip.h: mvlpt_op_conv2d)."""
    B, H, W, cin = x.shape
    cout = w_packed.shape[0]
    ho, wo = conv_out_size(H, k, stride), conv_out_size(W, k, stride)
    if out is None:
        out = torch.empty(B, ho, wo, cout, device=x.device, dtype=torch.float16)
    _lib.check(op_conv2d_raw(_req(x, torch.float16, "x"), w_packed, _req(scale, torch.float32, "scale"), _req(shift, torch.float32, "shift"),
                             resid, out, B, H, W, cin, cout, k, stride, relu), None, "op_conv2d")
    return out


def op_avgpool2x2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, H, W, c = x.shape
    if out is None:
        out = torch.empty(B, H // 2, W // 2, c, device=x.device, dtype=torch.float16)
    _lib.check(lib.mvlpt_op_avgpool2x2(_ptr(_req(x, torch.float16, "x")), _ptr(out), B, H, W, c, _stream()), None, "op_avgpool2x2")
    return out


def op_nchw_to_nhwc8(image: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    image = image.contiguous()
    B, _, R, _ = image.shape
    if out is None:
        out = torch.empty(B, R, R, 8, device=image.device, dtype=torch.float16)
    _lib.check(lib.mvlpt_op_nchw_to_nhwc8(_ptr(image), _TORCH2DT[image.dtype], _ptr(out), B, R, _stream()), None, "op_nchw_to_nhwc8")
    return out


def op_attnpool_tokens(x: torch.Tensor, pos: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, HW, E = x.shape
    if out is None:
        out = torch.empty(B, HW + 1, E, device=x.device, dtype=torch.float16)
    _lib.check(lib.mvlpt_op_attnpool_tokens(_ptr(_req(x, torch.float16, "x")), _ptr(_req(pos, torch.float32, "pos")), _ptr(out), B, HW, E,
                                            _stream()), None, "op_attnpool_tokens")
    return out


def op_attnpool_query(q: torch.Tensor, kv: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, T, E2 = kv.shape
    if out is None:
        out = torch.empty(B, E2 // 2, device=q.device, dtype=torch.float16)
    _lib.check(lib.mvlpt_op_attnpool_query(_ptr(_req(q, torch.float16, "q")), _ptr(_req(kv, torch.float16, "kv")), _ptr(out), B, T, E2 // 2,
                                           _stream()), None, "op_attnpool_query")
    return out
