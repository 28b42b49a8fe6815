"""What the schedule of a training step is made of (DESIGN.md "Step schedule"): which stream a tower is enqueued on and what is
kept from one forward to the next.  Three pieces, each the single owner of its state:

* `fork`: run a job on a second stream behind the current one and join it later — the one place that orders two streams;
* `ImagePrefetch`: the image towers computed ahead of the forward that uses them, on a stream of their own;
* `TextFeatureCache`: the text features that outlive a forward.

`mvlpt_amd.model.CustomCLIP` holds one of each of the last two, `_PromptedClipFn` asks them and forks, the trainer decides when
a prefetch starts.  Nothing here needs a GPU to import; with no second stream every caller runs its jobs inline."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from . import engine as _engine


def check_forward_is_current(model, generation: int) -> None:
    """The engine keeps ONE set of saved activations per tower: every forward takes the next `model._fwd_generation`, and a backward
    that arrives after another forward has overwritten them (gradient accumulation, test() between forward and backward) is refused
    instead of silently using the wrong activations."""
    if generation != model._fwd_generation:
        raise RuntimeError("backward of a stale forward: the engine holds the saved activations of the most recent "
                           "CustomCLIP.forward only (call backward before the next forward)")


def fork(stream, job: Callable, uses=()) -> Callable:
    """Run `job()` on `stream`, ordered behind everything the current stream holds; `uses`: tensors of the current stream that the
    job reads and that may be freed before it is done.  Returns the join: called on the same current stream it orders that stream
    behind the job and hands back the job's result (a tensor, or a tuple of tensors and None), safe to use and to free there."""
    main = torch.cuda.current_stream()
    stream.wait_stream(main)
    with torch.cuda.stream(stream):
        result = job()
    for t in uses:
        t.record_stream(stream)

    def join():
        main.wait_stream(stream)
        for t in (result if isinstance(result, tuple) else (result,)):
            if t is not None:
                t.record_stream(main)
        return result
    return join


class Prefetched(NamedTuple):
    """An image tower enqueued ahead.  `key`: ImagePrefetch.key of `image` when it was started; `features`: None while the tower is
    only begun; `ready`: behind everything enqueued for it so far; holding `image` pins its storage, so its pointer cannot be handed
    to another batch."""
    key: tuple
    features: Optional[torch.Tensor]
    ready: "torch.cuda.Event"
    image: torch.Tensor


class ImagePrefetch:
    """Image towers without visual prompts run ahead of the forward that uses them, on the prefetch stream, keyed by the image tensor
    they belong to.  A tensor's prefetch is *begun* (prefetch split: the first blocks only; the engine has one such tower at a time),
    *finished* (whole tower enqueued, features behind `ready`), then *picked up* by the forward of that tensor or *dropped*.
    All towers share the engine's one image workspace: they queue up on the one stream, and whoever runs a tower elsewhere waits for
    them first (`wait_for_writers`)."""

    KEEP = 4      # finished towers nobody picked up (a loop that reads ahead without consuming): the newest are kept

    def __init__(self, engine, device):
        self.engine, self.device = engine, device
        self.stream = None            # created on first use; CustomCLIP.set_cu_partition replaces it
        self.split = (0, 0)           # (stop_block, cu_cap) of TRAINER.MVLPT.PREFETCH_SPLIT; (0, 0): the tower in one piece
        self.begun = None             # the one tower begun and not resumed: a Prefetched without features
        self.finished = {}            # key -> Prefetched, oldest first

    @staticmethod
    def key(image):
        return image.data_ptr(), tuple(image.shape), image._version

    def get(self, image) -> Optional[Prefetched]:
        """The finished tower of `image`, if there is one; it stays here."""
        return self.finished.get(self.key(image))

    def _finish(self, key, image, features) -> None:
        """On the prefetch stream, behind the tower's last launch."""
        ready = torch.cuda.Event()
        ready.record(self.stream)
        if len(self.finished) >= self.KEEP:
            self.finished.pop(next(iter(self.finished)))
        self.finished[key] = Prefetched(key, features, ready, image)

    def finish_begun(self) -> None:
        """The rest of the tower that was begun: uncapped, on the prefetch stream."""
        begun = self.begun
        self.begun = None
        with torch.cuda.stream(self.stream):
            self._finish(begun.key, begun.image, self.engine.image_fwd_resume())

    def start(self, image, stop_block: int = 0, cu_cap: int = 0) -> None:
        """Start the tower of `image`, or continue it.  `stop_block` > 0 begins it: the tower entry and blocks [0, stop_block), their
        grids capped at `cu_cap` compute units (0: uncapped), so that they leave the rest of the chip to the text forward they run
        beside; the next call for the same tensor enqueues the rest behind whatever the current stream holds by then.  A tower begun
        for a tensor nobody came back for is finished first."""
        key = self.key(image)
        if key in self.finished:
            return
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        st = self.stream
        # the image tensor was produced (uploaded) on the current stream, and an image forward that ran there itself (no prefetch:
        # the first step, an evaluation) must be done with the tower workspace
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        st.wait_event(ready)
        if self.begun is not None:
            mine = self.begun.key == key
            self.finish_begun()
            if mine:
                return
        with torch.cuda.stream(st):
            if stop_block:
                _engine.set_stream_cu_cap(st, cu_cap)
                try:
                    self.engine.image_fwd_begin(image, None, None, save_for_bwd=False, stop_block=stop_block)
                finally:
                    _engine.set_stream_cu_cap(st, 0)
                first = torch.cuda.Event()
                first.record(st)
                self.begun = Prefetched(key, None, first, image)
            else:
                self._finish(key, image, self.engine.image_fwd(image, None, None, save_for_bwd=False))
        image.record_stream(st)

    def claim(self, image, prompted: bool) -> Optional[Prefetched]:
        """A forward over `image` is about to need its features: hand over this tensor's finished tower (to `pick_up`), or None
        after making the current stream wait for the towers of OTHER tensors, which are (or were) writing the workspace the forward
        will run its own tower in (they stay available to the forwards they were made for).  A tower begun for this tensor, or
        one nobody resumed (the loop left the loader early), is finished first: the engine has one image-tower state.  `prompted`:
        the forward has visual prompts and can use no prefetch."""
        key = self.key(image)
        if self.begun is not None and (prompted or key not in self.finished):
            self.finish_begun()
        entry = None if prompted else self.finished.pop(key, None)
        if entry is None:
            self.wait_for_writers()
        return entry

    @staticmethod
    def pick_up(entry: Prefetched) -> torch.Tensor:
        """The features of a claimed tower, on the current stream."""
        cur = torch.cuda.current_stream()
        cur.wait_event(entry.ready)
        entry.features.record_stream(cur)
        return entry.features

    def wait_for_writers(self) -> None:
        """The current stream waits for everything enqueued here that still writes the image-tower workspace."""
        if self.begun is not None:
            torch.cuda.current_stream().wait_event(self.begun.ready)
        for entry in self.finished.values():
            torch.cuda.current_stream().wait_event(entry.ready)

    def drop(self) -> None:
        """Forget every tower nobody will pick up (the loop left the loader early), with the workspace quiescent for whatever the
        current stream runs next.  A tower that was begun is given up: the next forward carves the workspace anew, behind its first part."""
        if self.begun is not None:
            self.engine.image_fwd_abandon()
        self.wait_for_writers()
        self.begun = None
        self.finished = {}


class TextFeatureCache:
    """The text features that outlive the forward that computed them.  A forward is in one of three states (`lookup`):

    * constants: the model has no text context, so the features depend on nothing trainable; computed once, kept
      across training steps;
    * evaluation: an inference forward; the features depend only on the prompt parameters and are kept per parameter version,
      instead of once per batch as the reference does (trainers/mvlpt.py:546-548 under test(), :989-1088);
    * none: a training forward with a text context runs the tower."""

    CONSTANTS = "constants"

    def __init__(self):
        self.constants = None
        self.eval_key = self.eval_features = None

    def lookup(self, prompt_learner, has_ctx: bool, need_grad: bool):
        """-> (features or None: run the tower, slot): `slot` says where the tower's result belongs (`store`), None for nowhere."""
        if not has_ctx:
            return self.constants, self.CONSTANTS
        if prompt_learner.training or need_grad:      # Dassl sets the mode on the registered prompt_learner
            return None, None
        key = tuple((id(p), p._version) for p in prompt_learner.parameters())
        return (self.eval_features if key == self.eval_key else None), key

    def store(self, slot, features, gathered: bool = False) -> None:
        """`gathered`: the features are a class-sharded tower's all-gather result, which lives in a buffer the next gather reuses, so
        the evaluation cache keeps a copy."""
        if slot == self.CONSTANTS:
            self.constants = features
        elif slot is not None:
            self.eval_key, self.eval_features = slot, (features.clone() if gathered else features)
