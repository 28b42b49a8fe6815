"""float64 numpy statement of the three update rules of the fused optimizer step (mvlpt_op_optim_step): torch.optim's single-tensor
SGD (momentum / dampening / nesterov, first-step buffer rule), Adam (L2 decay) and AdamW (decoupled decay), over a flat buffer cut
into segments with step counts of their own.  tests/test_optim_ref.py pins it against torch.optim in float64; the GPU tests
(tests/test_hip_optim.py, tests/test_hip_fused_trainer.py) compare the kernel with it.  Also the error terms of the GPU bound."""
import numpy as np

SGD, ADAM, ADAMW = 0, 1, 2


def sgd(p, g, buf, first, lr, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False):
    """One SGD step of one tensor; `first`: its first step (buf = d, no dampening).  Returns (p', buf'); buf' is `buf` for momentum 0."""
    d = g + wd * p
    if momentum == 0:
        return p - lr * d, buf
    buf = d.copy() if first else momentum * buf + (1.0 - dampening) * d
    return p - lr * (d + momentum * buf if nesterov else buf), buf


def adam(p, g, m, v, t, lr, wd=0.0, beta1=0.9, beta2=0.999, eps=1e-8, decoupled=False):
    """One Adam (decoupled: AdamW) step of one tensor that is on its t-th step (t >= 1).  Returns (p', m', v')."""
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps
    return p - (lr / (1.0 - beta1 ** t)) * m / denom, m, v


def flat_step(kind, hyper, param, grad, s1, s2, segs):
    """The launch: `segs` = [(begin, end, active, t)] with t the segment's own 1-based step count; float64 arrays in, new arrays out.
    Elements of inactive segments (and outside every segment) come back unchanged."""
    P, S1, S2 = param.copy(), None if s1 is None else s1.copy(), None if s2 is None else s2.copy()
    for b, e, active, t in segs:
        if not active:
            continue
        sl = slice(b, e)
        if kind == SGD:
            buf = None if s1 is None else s1[sl]
            P[sl], nb = sgd(param[sl], grad[sl], buf, t == 1, hyper["lr"], hyper.get("weight_decay", 0.0), hyper.get("momentum", 0.0),
                            hyper.get("dampening", 0.0), hyper.get("nesterov", False))
            if s1 is not None and hyper.get("momentum", 0.0) != 0:
                S1[sl] = nb
        else:
            P[sl], S1[sl], S2[sl] = adam(param[sl], grad[sl], s1[sl], s2[sl], t, hyper["lr"], hyper.get("weight_decay", 0.0),
                                         hyper.get("beta1", 0.9), hyper.get("beta2", 0.999), hyper.get("eps", 1e-8), kind == ADAMW)
    return P, S1, S2


class FlatOptimizer:
    """Several steps over a list of tensors, a tensor with `grad None` sitting a step out (its own step count does not advance)."""

    def __init__(self, kind, params, **hyper):
        self.kind, self.hyper = kind, hyper
        self.params = [np.asarray(p, np.float64).copy() for p in params]
        self.s1 = [np.zeros_like(p) for p in self.params]
        self.s2 = [np.zeros_like(p) for p in self.params]
        self.steps = [0] * len(self.params)

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            p, s1, s2 = flat_step(self.kind, self.hyper, self.params[i].ravel(), np.asarray(g, np.float64).ravel(), self.s1[i].ravel(),
                                  self.s2[i].ravel(), [(0, self.params[i].size, 1, self.steps[i])])
            self.params[i] = p.reshape(self.params[i].shape)
            if s1 is not None:
                self.s1[i] = s1.reshape(self.params[i].shape)
            if s2 is not None:
                self.s2[i] = s2.reshape(self.params[i].shape)


# ---- what enters each result, in absolute values: the GPU tests bound |kernel - reference| by k * 2^-24 * T per element
def sgd_terms(p, g, buf, first, lr, wd=0.0, momentum=0.0, dampening=0.0, nesterov=False):
    """(T_p, T_buf).  T_p = |p| + lr (|g| + wd |p|)(1 + m) + lr m (1 + m) |buf| covers every variant (nesterov included)."""
    d = np.abs(g) + wd * np.abs(p)
    b = np.zeros_like(p) if (first or momentum == 0) else np.abs(buf)
    return np.abs(p) + lr * d * (1 + momentum) + lr * momentum * (1 + momentum) * b, momentum * b + d


def adam_terms(p, g, m, v, t, lr, wd=0.0, beta1=0.9, beta2=0.999, eps=1e-8, decoupled=False):
    """(T_p, T_m, T_v): T_m = |m| + (1 - b1)(|g'| + |m|) (the kernel forms m + (1 - b1)(g' - m), as torch's lerp_), T_v = v',
    T_p = |p| (1 + lr wd) + step_size * T_m / denom."""
    gp = np.abs(g) + (0.0 if decoupled else wd * np.abs(p))
    Tm = np.abs(m) + (1.0 - beta1) * (gp + np.abs(m))
    Tv = beta2 * v + (1.0 - beta2) * gp * gp
    _, _, v1 = adam(p, g, m, v, t, lr, wd, beta1, beta2, eps, decoupled)
    denom = np.sqrt(v1) / np.sqrt(1.0 - beta2 ** t) + eps
    return np.abs(p) * (1.0 + lr * wd) + (lr / (1.0 - beta1 ** t)) * Tm / denom, Tm, Tv
