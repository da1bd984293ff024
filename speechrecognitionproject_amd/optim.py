"""Flat parameter/gradient buffers and the fused Adam of training.py:74,91 (srk_adam_step).

``FlatParams`` re-homes every parameter of a module into ONE contiguous fp32 buffer (each
tensor 256-byte aligned) and points ``p.grad`` at views of ONE gradient buffer, so that
  * the optimizer step is a single kernel launch over the whole model, and
  * the data-parallel gradient exchange is a single all-reduce of one buffer (parallel.py).
"""
import contextlib
import math

import torch

from ._lib import call, check_health, lib
from .features import ptr, require_gpu, stream_ptr

_ALIGN = 64   # floats


def flat_layout(params):
    """(order, offsets, numel) of a FlatParams buffer over `params`: the trainable parameters in their own order,
    an ``_srk_pair`` partner moved right behind its owner, every tensor starting on a multiple of 64 floats."""
    ps = [p for p in params if p.requires_grad]
    ids = {id(p) for p in ps}
    order, seen = [], set()
    for p in ps:
        if id(p) in seen:
            continue
        order.append(p)
        seen.add(id(p))
        q = getattr(p, "_srk_pair", None)
        if q is not None and id(q) in ids and id(q) not in seen:
            order.append(q)
            seen.add(id(q))
    offs, n = [], 0
    for p in order:
        offs.append(n)
        n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
    return order, offs, n


def decay_chunk_mask(params, offsets, numel, decay_filter):
    """One byte per 64-float chunk of a flat buffer (uint8, on the CPU): 1 where the chunk's parameter passes
    ``decay_filter``.  Every tensor starts on a chunk boundary, so a chunk belongs to one parameter; the padding
    behind a tensor shares its tensor's mark (it holds zeros and has zero gradients)."""
    assert numel % _ALIGN == 0 and all(o % _ALIGN == 0 for o in offsets)
    mask = torch.zeros(numel // _ALIGN, dtype=torch.uint8)
    for p, o in zip(params, offsets):
        if decay_filter(p):
            mask[o // _ALIGN:(o + p.numel() + _ALIGN - 1) // _ALIGN] = 1
    return mask


class FlatParams:
    def __init__(self, params, device=None):
        require_gpu()
        # a parameter may name a partner to be laid out right behind it (``_srk_pair``: the
        # reverse-direction twin of a BiGRU weight), so the kernels see the stacked pair as ONE
        # [2, ...] tensor in place — no per-step torch.stack / unbind copies
        self.params, offs, n = flat_layout(params)
        device = device or self.params[0].device
        self.numel = n
        self.offsets = offs
        self.data = torch.zeros(n, device=device, dtype=torch.float32)
        self.grad = torch.zeros(n, device=device, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                k = p.numel()
                self.data[o:o + k].copy_(p.data.reshape(-1))
                p.data = self.data[o:o + k].view_as(p)
                p.grad = self.grad[o:o + k].view_as(p)
                p._srk_flat = self    # the layers may accumulate into this .grad in place (nn.py)
        self._slot = {id(p): o for p, o in zip(self.params, offs)}

    def owns_grad(self, p):
        """p.grad is (still) this buffer's view for p."""
        o = self._slot.get(id(p))
        g = p.grad
        return (o is not None and g is not None and g.is_contiguous()
                and g.data_ptr() == self.grad.data_ptr() + o * self.grad.element_size())

    def zero_grad(self):
        self.grad.zero_()
        # autograd may have replaced a view with a fresh tensor; re-attach the views
        for p, o in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.grad[o:o + 1].data_ptr():
                p.grad = self.grad[o:o + p.numel()].view_as(p)


class LossScaler:
    """Loss scaling for fp16 training, torch.cuda.amp.GradScaler semantics with its state on the
    device (srk_grad_scaler_init, read by srk_adamw_step), so a captured HIP graph replays it:

        loss = criterion(model(x), y)
        scaler.scale(loss).backward()         # loss x scale (the scale is read on the device)
        optimizer.step(scaler=scaler)         # non-finite gradients -> the step is skipped

    ``dynamic=False`` keeps ``init_scale`` fixed (bench.py's static 1024); a skipped step is still
    counted in ``overflows()``.  ``dynamic=True`` halves the scale on an overflow and doubles it
    after ``growth_interval`` clean steps (GradScaler's defaults, except the initial scale)."""

    def __init__(self, init_scale=1024.0, dynamic=True, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, device=None):
        require_gpu()
        device = device or torch.device("cuda", torch.cuda.current_device())
        self.state = torch.zeros(8, dtype=torch.int32, device=device)
        self.dynamic = bool(dynamic)
        call("srk_grad_scaler_init", ptr(self.state), float(init_scale), float(growth_factor),
             float(backoff_factor), int(growth_interval) if dynamic else 0, stream_ptr())

    def scale(self, loss):
        return loss * self.state.view(torch.float32)[0]

    def get_scale(self):
        """The current scale (synchronizes)."""
        return float(self.state.view(torch.float32)[0].item())

    def overflows(self):
        """Steps skipped so far because a gradient was inf / NaN (synchronizes)."""
        return int(self.state[7].item())


def _default_decay_filter(p):
    return p.dim() >= 2


def _optr(t):
    """ptr() of an optional tensor: None (a null pointer) where it is absent."""
    return ptr(t) if t is not None else None


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (betas=(0.9, 0.999), eps=1e-8), one fused HIP launch per step over a FlatParams
    buffer.  ``grad_scale`` (e.g. 1/world_size after a summed all-reduce) multiplies the gradient inside the kernel;
    ``step(scaler=LossScaler)`` additionally unscales fp16 loss-scaled gradients and skips a step whose gradients
    overflowed.

    The step count lives on the device (``state_dev[0]``: a replayed HIP graph advances it without
    the host; a skipped step does not advance it); ``step_count`` reads it (synchronizes).

    Three optional extensions, all on the device and all replayed by a captured step (srk_adamw_step):
      * ``weight_decay`` > 0: torch.optim.AdamW's decoupled decay, ``p *= 1 - lr * weight_decay`` before the update,
        on the parameters ``decay_filter(p)`` accepts (default: two and more dimensions, so biases and
        normalisation parameters are left alone);
      * ``max_grad_norm``: torch.nn.utils.clip_grad_norm_ over all parameters (2-norm of the gradient after
        ``grad_scale`` and unscaling; one extra read of the gradient); ``last_grad_norm()`` and ``clipped_steps()``
        read the result (synchronize);
      * ``ema_decay``: ``ema = d * ema + (1 - d) * p`` after every step that is not skipped, in a buffer that starts
        as a copy of the parameters; ``with optimizer.ema_weights(): ...`` evaluates or saves the averaged weights.
    With all of them at their defaults, step() launches the same kernels and produces the same bits as without them:
    every configuration is one srk_adamw_step call, and what is off is a null pointer or a zero."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, flat=None, weight_decay=0.0,
                 decay_filter=_default_decay_filter, max_grad_norm=None, ema_decay=None):
        params = list(params)
        if not (weight_decay >= 0.0 and math.isfinite(weight_decay)):
            raise ValueError("weight_decay must be finite and >= 0, got %r" % (weight_decay,))
        if max_grad_norm is not None and not (max_grad_norm > 0.0 and math.isfinite(max_grad_norm)):
            raise ValueError("max_grad_norm must be a positive finite number or None, got %r" % (max_grad_norm,))
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError("ema_decay must be in [0, 1) or None, got %r" % (ema_decay,))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.flat = flat if flat is not None else FlatParams(params)
        self.exp_avg = torch.zeros_like(self.flat.data)
        self.exp_avg_sq = torch.zeros_like(self.flat.data)
        # {int64 step; float bc1, sqrt(bc2), lr, 0} on the device, so a captured HIP graph replays the
        # step count and follows lr changes (ExponentialLR) made between replays
        self.state_dev = torch.zeros(4, dtype=torch.int64, device=self.flat.data.device)
        self._lr_dev = None
        self.grad_scale = 1.0
        dev = self.flat.data.device
        self.weight_decay = float(weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        # the chunk mask is built once: one byte per 64 floats of the flat buffer
        self.decay_mask = None
        if self.weight_decay:
            self.decay_mask = decay_chunk_mask(self.flat.params, self.flat.offsets, self.flat.numel, decay_filter).to(dev)
        # {float total_norm, float coef, int32 clipped_steps, int32 0} and the norm pass's partial sums
        self.clip_state = self._norm_ws = None
        if self.max_grad_norm is not None:
            self.clip_state = torch.zeros(4, dtype=torch.int32, device=dev)
            self._norm_ws = torch.empty(int(lib().srk_adamw_workspace_floats(self.flat.numel)), dtype=torch.float32,
                                        device=dev)
        self.ema = self.flat.data.clone() if self.ema_decay is not None else None

    @property
    def step_count(self):
        return int(self.state_dev[0].item())

    def last_grad_norm(self):
        """The gradient's global 2-norm the last step measured, before clipping (synchronizes)."""
        self._need_clip()
        return float(self.clip_state.view(torch.float32)[0].item())

    def last_clip_coef(self):
        """What the last step multiplied the gradient by: min(1, max_grad_norm / (norm + 1e-6)) (synchronizes)."""
        self._need_clip()
        return float(self.clip_state.view(torch.float32)[1].item())

    def clipped_steps(self):
        """Steps so far (skipped ones not counted) whose gradient was scaled down (synchronizes)."""
        self._need_clip()
        return int(self.clip_state[2].item())

    def _need_clip(self):
        if self.clip_state is None:
            raise RuntimeError("this optimizer was made without max_grad_norm")

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model's parameters hold the averaged weights.  The CONTENTS of the flat buffer and
        of the EMA buffer are exchanged and exchanged back on exit: no tensor is re-pointed, so parameter views and
        captured graphs stay valid.  Not inside a stream capture."""
        if self.ema is None:
            raise RuntimeError("this optimizer was made without ema_decay")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ema_weights() exchanges buffers on the host's schedule: not inside a stream capture")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    @torch.no_grad()
    def _swap_ema(self):
        tmp = self.flat.data.clone()
        self.flat.data.copy_(self.ema)
        self.ema.copy_(tmp)

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    @torch.no_grad()
    def sync_lr(self):
        """Write param_groups[0]["lr"] into the device state if it changed (a captured step reads lr
        there: call this after an lr scheduler step when replaying a graph)."""
        lr = self.param_groups[0]["lr"]
        if lr != self._lr_dev and not torch.cuda.is_current_stream_capturing():
            self.state_dev.view(torch.float32)[4].fill_(float(lr))
            self._lr_dev = lr

    @torch.no_grad()
    def step(self, closure=None, scaler=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        f = self.flat
        self.sync_lr()
        # one entry for every configuration: what is off is a null pointer or a zero
        call("srk_adamw_step", ptr(f.data), ptr(f.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), f.numel,
             float(b1), float(b2), float(g["eps"]), ptr(self.state_dev), float(self.grad_scale),
             _optr(scaler.state if scaler is not None else None), self.weight_decay, _optr(self.decay_mask),
             self.max_grad_norm if self.max_grad_norm is not None else 0.0, _optr(self.clip_state),
             _optr(self.ema), self.ema_decay if self.ema_decay is not None else 0.0, _optr(self._norm_ws),
             stream_ptr())
        # a persistent kernel that timed out produced invalid gradients: fail loudly (a host-pinned
        # word, no device sync; it sees every timeout of the work the GPU has reached so far)
        check_health(sync=False)
        return loss
