"""Fused optimizer step: ONE HIP launch over the flat prompt buffers (mvlpt_op_optim_step, csrc/optim.hip).

`FusedSGD`, `FusedAdam` and `FusedAdamW` subclass the matching torch.optim classes: `param_groups`, `state_dict()` and
`load_state_dict()` keep torch's exact format, so a checkpoint written on this route resumes on the torch.optim route and the other
way round.  What differs is `step()`: the parameters' values are views of one buffer (distributed.FlatParameters), their gradients
views of a second (distributed.FlatGradients), the per-parameter state (`momentum_buffer`, or `exp_avg` / `exp_avg_sq`) views of a
third and fourth, and one kernel updates all of them.  A parameter whose `.grad is None` sits the step out untouched, as under
torch.optim.  There is no CPU path.

`step(loss_dev=...)` guards the update on the device: with a non-finite loss the launch writes nothing and counts itself in
`skipped_dev` (read it with `skipped()` where the host syncs anyway).  Such a launch still counts as a step of the schedule (Adam's
bias correction); the trainers stop at the next PRINT_FREQ check."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib
from .distributed import FlatGradients, FlatParameters


class _FusedStep:
    """Shared by the three classes: the flat state buffers, the segment table and its host mirror, the launch."""

    def _fused_init(self, kind: int, flat_params: FlatParameters, flat_grads: FlatGradients) -> None:
        if len(self.param_groups) != 1:
            raise ValueError("fused optimizers support one param group (no staged learning rates)")
        g = self.param_groups[0]
        for key in ("maximize", "amsgrad", "capturable", "differentiable"):
            if g.get(key, False):
                raise ValueError(f"fused optimizers do not support {key}=True")
        params = list(g["params"])
        if len(params) != len(flat_params.params) or any(a is not b for a, b in zip(params, flat_params.params)) or \
                len(params) != len(flat_grads.params) or any(a is not b for a, b in zip(params, flat_grads.params)):
            raise ValueError("fused optimizers step exactly the parameters of the FlatParameters / FlatGradients, in their order")
        if not params or not flat_params.flat.is_cuda:
            raise RuntimeError("fused optimizers need parameters on a HIP device: mvlpt_amd has no CPU path")
        if len(params) > _lib.OPTIM_MAX_SEGS:
            raise ValueError(f"fused optimizers take at most {_lib.OPTIM_MAX_SEGS} parameter tensors")
        self._kind, self._fp, self._fg, self._params = kind, flat_params, flat_grads, params
        dev = flat_params.flat.device
        n = flat_params.flat.numel()
        self._state1 = torch.zeros(n, dtype=torch.float32, device=dev) if (kind != _lib.OPTIM_SGD or g["momentum"] != 0) else None
        self._state2 = torch.zeros(n, dtype=torch.float32, device=dev) if kind != _lib.OPTIM_SGD else None
        bounds = [(o, o + p.numel()) for o, p in zip(flat_params.offsets, params)]
        self._view1 = [None if self._state1 is None else self._state1[b:e].view(p.shape) for (b, e), p in zip(bounds, params)]
        self._view2 = [None if self._state2 is None else self._state2[b:e].view(p.shape) for (b, e), p in zip(bounds, params)]
        self._step_t = torch.zeros(len(params), dtype=torch.float32)     # Adam's per-parameter `step` tensors are views of this one
        self._steps: List[int] = [0] * len(params)                        # host mirror: steps each parameter has taken
        self._launch = 0
        self._segs_host = (_lib.MvlptOptimSeg * len(params))()
        for s, (b, e) in zip(self._segs_host, bounds):
            s.begin, s.end, s.active, s.missed = b, e, 0, 0
        self._segs_dev = torch.zeros(C.sizeof(self._segs_host), dtype=torch.uint8, device=dev)
        self._active = None                                               # the active set the device table holds
        self._active_params, self._active_mask = [], None
        self.skipped_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._hyper = _lib.MvlptOptimHyper()
        self._pptr = [v.data_ptr() for v in flat_params.views]
        self._gptr = [v.data_ptr() for v in flat_grads.views]

    def add_param_group(self, param_group) -> None:
        if getattr(self, "_kind", None) is not None:
            raise ValueError("fused optimizers support one param group")
        super().add_param_group(param_group)

    # -- torch's state layout on the flat buffers
    def _publish_state(self, i: int) -> None:
        """state[p] of a parameter that has taken a step, in torch.optim's format, as views of the flat state buffers."""
        p = self._params[i]
        if self._kind == _lib.OPTIM_SGD:
            if self._state1 is not None:
                self.state[p]["momentum_buffer"] = self._view1[i]
        else:
            st = self.state[p]
            st["step"], st["exp_avg"], st["exp_avg_sq"] = self._step_t[i], self._view1[i], self._view2[i]

    def load_state_dict(self, state_dict) -> None:
        """torch's load_state_dict, then the loaded tensors are COPIED into the flat state buffers: the views stay."""
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("fused optimizers support one param group")
        loaded = self.state
        steps = []
        for i, p in enumerate(self._params):
            st = loaded.get(p, {})
            if self._kind == _lib.OPTIM_SGD:
                buf = st.get("momentum_buffer")
                if buf is not None and self._state1 is not None:
                    self._view1[i].copy_(buf)
                steps.append(0 if buf is None else 1)      # SGD only tells the first step from the later ones
            else:
                if "exp_avg" in st:
                    self._view1[i].copy_(st["exp_avg"])
                    self._view2[i].copy_(st["exp_avg_sq"])
                    steps.append(int(float(st["step"])))
                else:
                    steps.append(0)
        self._steps = steps
        self._step_t.copy_(torch.tensor(steps, dtype=torch.float32))
        self._launch = max(steps)
        self._active = None                                # table re-uploaded on the next step
        for i, p in enumerate(self._params):
            self.state.pop(p, None)
            if steps[i] > 0:
                self._publish_state(i)
        for s, k in zip(self._segs_host, steps):
            s.missed = self._launch - k

    def skipped(self) -> int:
        """Launches the loss guard has skipped so far (a device read: synchronises)."""
        return int(self.skipped_dev.item())

    @torch.no_grad()
    def step(self, closure=None, loss_dev: Optional[torch.Tensor] = None):
        if closure is not None:
            raise ValueError("fused optimizers take no closure")
        params = self._params
        # the active set, and whether every value / gradient still is its view (a first backward creates a tensor of its own)
        active, adopt = [], False
        for i, p in enumerate(params):
            g = p.grad
            active.append(g is not None)
            if p.data_ptr() != self._pptr[i] or (g is not None and g.data_ptr() != self._gptr[i]):
                adopt = True
        if adopt:
            self._fp.attach()
            self._fg.attach()
        self._launch += 1
        upload = active != self._active
        for i, a in enumerate(active):
            if a:
                missed = self._launch - self._steps[i] - 1     # launches this parameter sat out
                if self._steps[i] == 0:
                    self._publish_state(i)
                self._steps[i] += 1
                s = self._segs_host[i]
                if s.missed != missed:                         # it comes back after sitting out
                    s.missed, upload = missed, True
        if upload:
            for s, a in zip(self._segs_host, active):
                s.active = int(a)
            self._active = active
            self._active_params = [p for p, a in zip(params, active) if a]
            self._active_mask = torch.tensor([float(a) for a in active])
            # stream-ordered copy from a fresh pageable tensor: only when the active set changes, never in the steady state
            self._segs_dev.copy_(torch.frombuffer(bytearray(self._segs_host), dtype=torch.uint8))
        if not self._active_params:
            return None
        g = self.param_groups[0]
        h = self._hyper
        h.kind, h.lr, h.weight_decay, h.launch = self._kind, float(g["lr"]), float(g["weight_decay"]), self._launch
        if self._kind == _lib.OPTIM_SGD:
            h.momentum, h.dampening, h.nesterov = float(g["momentum"]), float(g["dampening"]), int(bool(g["nesterov"]))
        else:
            h.beta1, h.beta2, h.eps = float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        if loss_dev is not None and (loss_dev.dtype != torch.float32 or loss_dev.device != self._fp.flat.device or loss_dev.numel() != 1):
            raise ValueError("loss_dev: one fp32 value on the parameters' device")
        with torch.cuda.device(self._fp.flat.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib.mvlpt_op_optim_step(
                C.byref(h), self._fp.flat.data_ptr(), self._fg.flat.data_ptr(),
                None if self._state1 is None else self._state1.data_ptr(), None if self._state2 is None else self._state2.data_ptr(),
                self._fp.flat.numel(), self._segs_dev.data_ptr(), len(params),
                None if loss_dev is None else loss_dev.data_ptr(), self.skipped_dev.data_ptr(), stream), None, "op_optim_step")
        if self._kind != _lib.OPTIM_SGD:
            self._step_t += self._active_mask
        # the kernel wrote behind autograd's back: whoever keys a cache on p._version (the evaluation text features) must see it
        torch.autograd.graph.increment_version(self._active_params)
        return None


class FusedSGD(_FusedStep, torch.optim.SGD):
    def __init__(self, flat_params: FlatParameters, flat_grads: FlatGradients, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False):
        torch.optim.SGD.__init__(self, flat_params.params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                 nesterov=nesterov)
        self._fused_init(_lib.OPTIM_SGD, flat_params, flat_grads)


class FusedAdam(_FusedStep, torch.optim.Adam):
    def __init__(self, flat_params: FlatParameters, flat_grads: FlatGradients, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False):
        if amsgrad:
            raise ValueError("fused optimizers do not support amsgrad=True")
        torch.optim.Adam.__init__(self, flat_params.params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._fused_init(_lib.OPTIM_ADAM, flat_params, flat_grads)


class FusedAdamW(_FusedStep, torch.optim.AdamW):
    def __init__(self, flat_params: FlatParameters, flat_grads: FlatGradients, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 amsgrad=False):
        if amsgrad:
            raise ValueError("fused optimizers do not support amsgrad=True")
        torch.optim.AdamW.__init__(self, flat_params.params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._fused_init(_lib.OPTIM_ADAMW, flat_params, flat_grads)


FUSED = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}
