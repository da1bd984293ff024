"""Autograd modules over libsrk.so: the drop-in replacements for the torch.nn layers the
reference models use (nn.GRU, nn.Linear, nn.CrossEntropyLoss).  Parameter names and shapes are
torch's, so reference ``state_dict`` checkpoints load unchanged.

Every forward/backward runs a HIP kernel through the C ABI; there is no CPU or torch-kernel
fallback (the GPU and the library are required).
"""
import ctypes
import math
import os

import torch
import torch.nn as tnn

from . import _lib
from ._lib import call
from .features import ptr, require_gpu, stream_ptr


def _optr(t):
    """ptr(t) of an optional tensor: None stays None (a null pointer across the C ABI)."""
    return None if t is None else ptr(t)


def _check_cuda(*ts):
    for t in ts:
        if t is not None and (t.device.type != "cuda" or t.dtype != torch.float32):
            raise _lib.SrkError("libsrk ops need float32 CUDA tensors, got %s %s" % (t.device, t.dtype))


# ----------------------------------------------------------------------------- GRU
def _adjacent(a, b):
    """b starts right where a ends in one storage (FlatParams lays BiGRU twins out this way)."""
    return (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.shape == b.shape
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size())


def _dir_pair(a, b):
    """The [2, ...] stacked tensor of a direction pair: a view when adjacent, else a copy."""
    if _adjacent(a, b):
        return a.as_strided((2,) + tuple(a.shape), (a.numel(),) + tuple(a.stride()))
    return torch.stack([a, b])


# conv weight / BatchNorm parameter gradients added into FlatParams-owned .grad by their kernels (A/B switch:
# 0 = returned to autograd; the GRU's in-place pairs are not affected)
INPLACE_GRADS = os.environ.get("SRK_INPLACE_GRADS", "1") != "0"


def _flat_grad(p):
    """p.grad when p is owned by a FlatParams (optim.py) and its .grad is still that buffer's view:
    the one case where a backward may accumulate into .grad in place (beta = 1 in the GEMM
    epilogue) and hand autograd None.  Any other parameter (plain torch optimizers, DDP,
    torch.autograd.grad) gets its gradient returned to autograd as usual, so AccumulateGrad and
    its hooks run."""
    flat = getattr(p, "_srk_flat", None)
    g = p.grad
    if flat is None or g is None or not flat.owns_grad(p):
        return None
    return g


def _reducer_of(p):
    """The overlapped gradient all-reduce (parallel.GradReducer) attached to p's FlatParams, if any."""
    flat = getattr(p, "_srk_flat", None)
    return getattr(flat, "reducer", None) if flat is not None else None


def _grad_pair(a, b):
    """The stacked .grad of a FlatParams-owned direction pair to ACCUMULATE into in place
    (autograd's own accumulation, fused into the kernels' epilogues), or None (then the gradient
    is returned to autograd as usual)."""
    ga, gb = _flat_grad(a), _flat_grad(b)
    if ga is None or gb is None or not _adjacent(ga, gb):
        return None
    return _dir_pair(ga, gb)


class _GRULayerFn(torch.autograd.Function):
    """One bidirectional GRU layer (srk_gru_layer_fwd / srk_gru_layer_bwd) over the direction
    pairs (weight_ih_lN, weight_ih_lN_reverse), ... of the parameters themselves."""

    @staticmethod
    def forward(ctx, x, grad_on, *params):
        (B, T, IN, H), x, pairs, y, ws, x16 = _gru_operands(x, params, "srk_gru_workspace_floats")
        call("srk_gru_layer_fwd_x16", ptr(x), _optr(x16), B, T, IN, H, *map(ptr, pairs), ptr(y), ptr(ws), stream_ptr())
        # this layer's 16-bit copy of its output goes to the next layer
        off = int(_lib.lib().srk_gru_y16_offset(B, T, IN, H)) if _copy16_wanted(2 * H) else -1
        if off >= 0 and grad_on and any(ctx.needs_input_grad):
            _copy16_put(y, ws[off:].view(torch.int16)[:y.numel()])
        _gru_forward_done(ctx, grad_on, (B, T, IN, H), x, pairs, y, ws, x16, params)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x, w_ih, w_hh, y, ws), (B, T, IN, H), dx, grads, acc, ws2 = _gru_backward_buffers(
            ctx, "srk_gru_workspace_floats")
        _copy16_drop(y)   # the next layer's backward has run
        dy = dy.contiguous()
        x16, ctx.x16 = ctx.x16, None
        with _lib.precision_scope(ctx.prec):
            call("srk_gru_layer_bwd_x16", ptr(x), _optr(x16), B, T, IN, H, ptr(w_ih), ptr(w_hh), ptr(y), ptr(ws),
                 ptr(dy), _optr(dx), *map(ptr, grads), int(acc), ptr(ws2), stream_ptr())
        return _gru_backward_done(ctx, dx, grads, acc)


class _GRUTopLastFn(torch.autograd.Function):
    """The top BiGRU layer of a model that reads only the last step (srk_gru_top_last_fwd / _bwd): returns row T-1
    of the layer, [B, 2H], and takes dy_last [B, 2H] in backward.  Everything around the kernels is _GRULayerFn's
    (the _gru_* helpers below).  The full y is kept for the backward only and never returned (in the library's
    modes 2 and 3 its reverse half is unwritten below the last step)."""

    @staticmethod
    def forward(ctx, x, grad_on, *params):
        (B, T, IN, H), x, pairs, y, ws, x16 = _gru_operands(x, params, "srk_gru_top_last_workspace_floats")
        y_last = torch.empty((B, 2 * H), device=x.device, dtype=torch.float32)
        mode = ctypes.c_int(0)
        call("srk_gru_top_last_fwd", ptr(x), _optr(x16), B, T, IN, H, *map(ptr, pairs), ptr(y), ptr(y_last), ptr(ws),
             ctypes.byref(mode), stream_ptr())
        ctx.mode = mode.value
        _gru_forward_done(ctx, grad_on, (B, T, IN, H), x, pairs, y, ws, x16, params)
        return y_last

    @staticmethod
    def backward(ctx, dy_last):
        (x, w_ih, w_hh, y, ws), (B, T, IN, H), dx, grads, acc, ws2 = _gru_backward_buffers(
            ctx, "srk_gru_top_last_workspace_floats")
        dy_last = dy_last.contiguous()
        x16, ctx.x16 = ctx.x16, None
        with _lib.precision_scope(ctx.prec):
            call("srk_gru_top_last_bwd", ptr(x), _optr(x16), B, T, IN, H, ptr(w_ih), ptr(w_hh), ptr(y), ptr(ws),
                 ptr(dy_last), ctx.mode, _optr(dx), *map(ptr, grads), int(acc), ptr(ws2), stream_ptr())
        return _gru_backward_done(ctx, dx, grads, acc)


# What _GRULayerFn and _GRUTopLastFn share around their library calls.  params: the eight parameters of the layer,
# (weight_ih, weight_ih_reverse, weight_hh, ..., bias_hh_reverse); grad_on: torch.is_grad_enabled() at the call
# (inside forward it is always off, and needs_input_grad ignores it): an evaluation pass under no_grad must not
# register copies or hold the reducer back.
def _gru_operands(x, params, ws_floats):
    """The forward's operands: dims, contiguous x, the direction pairs (w_ih, w_hh, b_ih, b_hh), y, the workspace and,
    in 16-bit modes, the previous layer's own 16-bit copy of h as this layer's x16 (module note at _copies16)."""
    B, T, IN = x.shape
    H = params[2].shape[-1]
    x = x.contiguous()
    pairs = tuple(_dir_pair(params[2 * i], params[2 * i + 1]) for i in range(4))
    _check_cuda(x, *pairs)
    y = torch.empty((B, T, 2 * H), device=x.device, dtype=torch.float32)
    ws = torch.empty(int(getattr(_lib.lib(), ws_floats)(B, T, IN, H, 0)), device=x.device)
    x16 = _copy16_get(x) if IN % 8 == 0 else None
    return (B, T, IN, H), x, pairs, y, ws, x16


def _gru_forward_done(ctx, grad_on, dims, x, pairs, y, ws, x16, params):
    ctx.x16 = x16
    ctx.save_for_backward(x, pairs[0], pairs[1], y, ws)
    ctx.dims = dims
    ctx.params = params
    ctx.prec = _lib.matmul_precision()   # the backward runs at its forward's precision
    red = _reducer_of(params[0])
    if red is not None and grad_on and any(ctx.needs_input_grad):
        red.persistent_pending(1)      # collectives wait until this layer's recurrence is enqueued


def _gru_backward_buffers(ctx, ws_floats):
    """(saved tensors, dims, dx or None, (dw_ih, dw_hh, db_ih, db_hh), acc, the backward workspace).  acc: the four
    gradients are the parameters' own stacked .grad (FlatParams), accumulated into in place."""
    x, w_ih, w_hh, y, ws = ctx.saved_tensors
    B, T, IN, H = ctx.dims
    P = ctx.params
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    grads = [_grad_pair(P[2 * i], P[2 * i + 1]) for i in range(4)]
    acc = all(t is not None for t in grads) and all(ctx.needs_input_grad[2:])
    if not acc:
        grads = [torch.empty_like(w_ih), torch.empty_like(w_hh), torch.empty((2, 3 * H), device=x.device),
                 torch.empty((2, 3 * H), device=x.device)]
    ws2 = torch.empty(int(getattr(_lib.lib(), ws_floats)(B, T, IN, H, 1)), device=x.device)
    return (x, w_ih, w_hh, y, ws), ctx.dims, dx, grads, acc, ws2


def _gru_backward_done(ctx, dx, grads, acc):
    """The reducer hand-shake and backward's return tuple: None for gradients accumulated in place."""
    red = _reducer_of(ctx.params[0])
    if red is not None:
        red.persistent_done()
        if acc:
            red.mark_ready(ctx.params)
    if acc:
        return (dx, None) + (None,) * 8
    return (dx, None) + tuple(g[d] for g in grads for d in (0, 1))


class BiGRU(tnn.Module):
    """Drop-in for ``nn.GRU(input_size, hidden_size, num_layers, bidirectional=True,
    batch_first=True)`` (h0 = 0, no inter-layer dropout).  ``forward(x) -> (output, h_n)``."""

    def __init__(self, input_size, hidden_size, num_layers=1, bidirectional=True, batch_first=True):
        super().__init__()
        if not (bidirectional and batch_first):
            raise ValueError("BiGRU implements bidirectional=True, batch_first=True (the reference's config)")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bidirectional, self.batch_first = True, True
        H = hidden_size
        k = 1.0 / H ** 0.5
        for layer in range(num_layers):
            inp = input_size if layer == 0 else 2 * H
            for sfx in ("", "_reverse"):
                for name, shape in (("weight_ih", (3 * H, inp)), ("weight_hh", (3 * H, H)),
                                    ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,))):
                    p = tnn.Parameter(torch.empty(shape).uniform_(-k, k))
                    setattr(self, "%s_l%d%s" % (name, layer, sfx), p)
            for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):   # FlatParams layout hint
                getattr(self, "%s_l%d" % (name, layer))._srk_pair = getattr(self, "%s_l%d_reverse" % (name, layer))

    def _pairs(self, layer):
        return [getattr(self, "%s_l%d%s" % (name, layer, sfx))
                for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for sfx in ("", "_reverse")]

    def forward(self, x):
        require_gpu()
        h = x
        finals = []
        for layer in range(self.num_layers):
            h = _GRULayerFn.apply(h, torch.is_grad_enabled(), *self._pairs(layer))
            H = self.hidden_size
            finals += [h[:, -1, :H], h[:, 0, H:]]
        return h, torch.stack(finals)

    def forward_last(self, x):
        """``forward(x)[0][:, -1, :]`` -> [B, 2H] for the models that read nothing else (fc on the last step):
        the top layer computes only what that row needs (_GRUTopLastFn); no h_n is built."""
        require_gpu()
        h = x
        for layer in range(self.num_layers - 1):
            h = _GRULayerFn.apply(h, torch.is_grad_enabled(), *self._pairs(layer))
        return _GRUTopLastFn.apply(h, torch.is_grad_enabled(), *self._pairs(self.num_layers - 1))


class _LastStepFn(torch.autograd.Function):
    """``x[:, -1, :]`` of a [B, T, C] sequence — the models' last-step select before their fc layer
    (model_mfcc_bgru.py:37 and the other BiGRU plugins).  The forward is the same strided view (the Linear
    GEMM reads it by row stride); the backward writes the [B, T, C] gradient, zeros and the last step, in
    one pad kernel instead of autograd's zero fill followed by a slice copy (one launch less per step)."""

    @staticmethod
    def forward(ctx, x):
        ctx.T = x.shape[1]
        return x[:, -1, :]

    @staticmethod
    def backward(ctx, g):
        return tnn.functional.pad(g.unsqueeze(1), (0, 0, ctx.T - 1, 0))


def last_step(x):
    """``x[:, -1, :]`` with a one-kernel backward (``_LastStepFn``)."""
    return _LastStepFn.apply(x)


# ----------------------------------------------------------------------------- attention pooling
class _AttentionPoolFn(torch.autograd.Function):
    """srk_attn_pool_fwd / _bwd: alpha = softmax_t(scale <q, y_t>), ctx = sum_t alpha_t y_t.  fp32 at every
    matmul precision (a softmax, like the loss); alpha is an output only."""

    @staticmethod
    def forward(ctx, y, q, scale):
        y, q = y.contiguous(), q.contiguous()
        _check_cuda(y, q)
        if y.dim() != 3 or q.shape != (y.shape[0], y.shape[2]):
            raise _lib.SrkError("attention pool: y must be [B, T, D] and q [B, D], got %s and %s"
                                % (tuple(y.shape), tuple(q.shape)))
        B, T, D = y.shape
        out = torch.empty((B, D), device=y.device)
        alpha = torch.empty((B, T), device=y.device)
        call("srk_attn_pool_fwd", ptr(y), ptr(q), B, T, D, scale, ptr(out), ptr(alpha), stream_ptr())
        ctx.save_for_backward(y, q, alpha)
        ctx.scale = scale
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, dctx, _dalpha):
        y, q, alpha = ctx.saved_tensors
        B, T, D = y.shape
        dctx = dctx.contiguous()
        dy, dq = torch.empty_like(y), torch.empty_like(q)
        call("srk_attn_pool_bwd", ptr(y), ptr(q), ptr(alpha), ptr(dctx), B, T, D, ctx.scale, ptr(dy), ptr(dq),
             stream_ptr())
        return dy, dq, None


class AttentionPool(tnn.Module):
    """Attention pooling over time: ``forward(y [B, T, D], q [B, D]) -> (ctx [B, D], alpha [B, T])`` with
    alpha = softmax over t of scale * <q, y_t> and ctx = sum_t alpha_t y_t, in one fused kernel each way.
    ``scale`` defaults to 1 / sqrt(D).  No parameters; gradients flow to y and q, not into alpha (the per-step
    weights are there to be looked at)."""

    def __init__(self, scale=None):
        super().__init__()
        self.scale = scale

    def forward(self, y, q):
        require_gpu()
        scale = float(self.scale) if self.scale is not None else y.shape[-1] ** -0.5
        return _AttentionPoolFn.apply(y, q, scale)


# ----------------------------------------------------------------------------- PCEN
class _PCENFn(torch.autograd.Function):
    """srk_pcen_fwd / _bwd (include/srk.h): fp32 at every matmul precision.  The gradient of ``params`` is with
    respect to the raw rows (the library applies exp' / sigmoid'), returned to autograd."""

    @staticmethod
    def forward(ctx, x, params, log_scale, eps, grad_on, ws):
        # grad_on: torch.is_grad_enabled() at the call (always off in here): evaluation passes keep no M
        x, p = x.contiguous(), params.contiguous()
        _check_cuda(x, p)
        if x.dim() != 3 or p.shape != (4, x.shape[2]):
            raise _lib.SrkError("PCEN: x must be [B, T, C] and params [4, C], got %s and %s"
                                % (tuple(x.shape), tuple(p.shape)))
        B, T, C = x.shape
        y = torch.empty_like(x)
        m = torch.empty_like(x) if grad_on and any(ctx.needs_input_grad[:2]) else None
        call("srk_pcen_fwd", ptr(x), ptr(p), B, T, C, log_scale, eps, ptr(y), _optr(m),
             stream_ptr())
        if m is not None:
            ctx.save_for_backward(x, p, m)
        ctx.consts = (log_scale, eps, ws)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, p, m = ctx.saved_tensors
        log_scale, eps, ws = ctx.consts
        B, T, C = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dp = torch.empty_like(p)
        call("srk_pcen_bwd", ptr(x), ptr(p), ptr(m), ptr(dy), B, T, C, log_scale, eps,
             _optr(dx), ptr(dp), ptr(ws), stream_ptr())
        return dx, dp, None, None, None, None


class PCEN(tnn.Module):
    """Trainable per-channel energy normalisation (Wang et al., ICASSP 2017) over ``x [B, T, C]``:
    ``E = exp(log_scale x)`` (``log_scale`` 0: ``E = x``), ``M[0] = E[0]``, ``M[t] = (1 - s) M[t-1] + s E[t]``,
    ``y = (E / (eps + M)^alpha + delta)^r - delta^r``, one fused kernel each way.  ``log_scale`` defaults to
    ln(10) / 20, the inverse of K2's ``20 log10``; 1 serves K3's natural log.

    One parameter ``params`` [4, C]: rows log alpha, log delta, log r, logit s (so every constant keeps its
    sign and s stays in (0, 1) under any optimizer step), initialised from the constructor's values, the
    paper's.  ``constants()`` returns the effective per-channel vectors."""

    def __init__(self, num_channels, log_scale=math.log(10.0) / 20.0, eps=1e-6, alpha=0.98, delta=2.0, r=0.5, s=0.025):
        super().__init__()
        if not (alpha > 0 and delta > 0 and r > 0 and 0 < s < 1 and eps > 0):
            raise ValueError("PCEN needs alpha, delta, r, eps > 0 and 0 < s < 1")
        self.num_channels, self.log_scale, self.eps = int(num_channels), float(log_scale), float(eps)
        rows = torch.tensor([math.log(alpha), math.log(delta), math.log(r), math.log(s / (1.0 - s))],
                            dtype=torch.float64)
        self.params = tnn.Parameter(rows.unsqueeze(1).repeat(1, self.num_channels).float())
        self._ws = {}

    def constants(self):
        """{"alpha", "delta", "r", "s"}: the effective per-channel constants, detached [C] tensors."""
        with torch.no_grad():
            p = self.params.detach()
            return {"alpha": p[0].exp(), "delta": p[1].exp(), "r": p[2].exp(), "s": torch.sigmoid(p[3])}

    def _workspace(self, x):
        # one buffer per (device, shape), kept for the module's life: a captured step keeps its address
        key = (x.device.index,) + tuple(x.shape)
        ws = self._ws.get(key)
        if ws is None:
            n = int(_lib.lib().srk_pcen_workspace_floats(*x.shape))
            ws = self._ws[key] = torch.empty(n, device=x.device)
        return ws

    def forward(self, x):
        require_gpu()
        grad_on = torch.is_grad_enabled()
        ws = self._workspace(x) if grad_on and x.dim() == 3 else None
        return _PCENFn.apply(x, self.params, self.log_scale, self.eps, grad_on, ws)


# ----------------------------------------------------------------------------- Linear
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        # x may be a row-strided 2-D view (e.g. out[:, -1, :]); the GEMM takes its row stride
        if x.dim() != 2 or x.stride(1) != 1:
            x = x.contiguous()
        _check_cuda(x, w, b)
        w_param = w
        w = w.contiguous()
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty((M, N), device=x.device)
        call("srk_gemm_f32", 0, 1, M, N, K, 1.0, ptr(x), x.stride(0), ptr(w), K, 0.0, ptr(y), N,
             _optr(b), 1 if b is not None else 0, stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.params = (w_param, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        M, K = x.shape
        N = w.shape[0]
        dx = dw = db = None
        s = stream_ptr()
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, K), device=x.device)
            call("srk_gemm_f32", 0, 0, M, K, N, 1.0, ptr(dy), N, ptr(w), K, 0.0, ptr(dx), K, None, 0, s)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        # accumulate straight into the parameters' existing .grad buffers (beta = 1, fused into the
        # GEMM epilogue) instead of returning a fresh gradient for autograd to add
        wp, bp = ctx.params
        gw = _flat_grad(wp)
        gb = _flat_grad(bp) if bp is not None else None
        acc = gw is not None and (not want_db or gb is not None)
        if ctx.needs_input_grad[1]:
            dw = gw if acc else torch.empty((N, K), device=x.device)
            beta = 1.0 if acc else 0.0
            if want_db:   # dW = dy^T x with db = row sums of dy^T fused into the same kernel
                db = gb if acc else torch.empty((N,), device=x.device)
                call("srk_gemm_rowsum_f32", 1, 0, N, K, M, 1.0, ptr(dy), N, ptr(x), x.stride(0), beta, ptr(dw), K,
                     ptr(db), s)
            else:
                call("srk_gemm_f32", 1, 0, N, K, M, 1.0, ptr(dy), N, ptr(x), x.stride(0), beta, ptr(dw), K, None, 0,
                     s)
        else:
            acc = False
        if want_db and db is None:
            db = torch.empty((N,), device=x.device)
            call("srk_colsum_f32", ptr(dy), M, N, N, ptr(db), 0.0, s)
        if acc:
            red = _reducer_of(wp)
            if red is not None:
                red.mark_ready([wp] + ([bp] if bp is not None else []))
            return dx, None, None
        return dx, dw, db


class Linear(tnn.Module):
    """Drop-in for ``nn.Linear`` (same parameter names/shapes/init)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = tnn.Parameter(torch.empty(out_features, in_features))
        self.bias = tnn.Parameter(torch.empty(out_features)) if bias else None
        ref = tnn.Linear(in_features, out_features, bias)     # torch's own init distribution
        with torch.no_grad():
            self.weight.copy_(ref.weight)
            if bias:
                self.bias.copy_(ref.bias)

    def forward(self, x):
        require_gpu()
        lead = x.shape[:-1]
        y = _LinearFn.apply(x.reshape(-1, x.shape[-1]) if x.dim() != 2 else x, self.weight, self.bias)
        return y.reshape(*lead, self.out_features)


# ----------------------------------------------------------------------------- loss
class _CrossEntropyFn(torch.autograd.Function):
    """The loss on the hard target (srk_cross_entropy), or with a mix (partner, lam) and / or smoothing on the soft
    target (srk_cross_entropy_mix): one kernel behind both, each entry with its own error texts."""

    @staticmethod
    def forward(ctx, logits, labels, partner, lam, smoothing):
        logits = logits.contiguous()
        _check_cuda(logits)
        B, C = logits.shape
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        if partner is not None:
            partner = torch.as_tensor(partner).to(device=logits.device, dtype=torch.int32).contiguous()
            lam = torch.as_tensor(lam).to(device=logits.device, dtype=torch.float32).contiguous()
            if tuple(partner.shape) != (B,) or tuple(lam.shape) != (B,):
                raise _lib.SrkError("CrossEntropyLoss: mix = (partner, lam) must hold one value per row (%d), got %s "
                                    "and %s" % (B, tuple(partner.shape), tuple(lam.shape)))
        loss = torch.empty((), device=logits.device)
        dlogits = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        ws = torch.empty(B + 1, device=logits.device)
        if partner is None and lam is None and smoothing == 0.0:
            call("srk_cross_entropy", ptr(logits), ptr(labels), B, C, ptr(loss), _optr(dlogits), ptr(ws), stream_ptr())
        else:
            call("srk_cross_entropy_mix", ptr(logits), ptr(labels), _optr(partner), _optr(lam), B, C, float(smoothing),
                 ptr(loss), _optr(dlogits), ptr(ws), stream_ptr())
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None, None, None


class CrossEntropyLoss(tnn.Module):
    """Drop-in for ``nn.CrossEntropyLoss()`` (mean reduction), training.py:73.  ``label_smoothing`` is torch's
    (0 <= eps < 1); ``forward(.., mix=(partner, lam))`` takes the loss on a mixed batch's soft target, row b's
    target being lam[b] of its own label and 1 - lam[b] of row partner[b]'s (features.mixup_draw), smoothed after.
    Without either it is srk_cross_entropy as before."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:
            raise ValueError("CrossEntropyLoss: label_smoothing must be in [0, 1), got %r" % (label_smoothing,))
        self.label_smoothing = eps

    def forward(self, logits, labels, mix=None):
        require_gpu()
        partner, lam = (None, None) if mix is None else mix
        return _CrossEntropyFn.apply(logits, labels, partner, lam, self.label_smoothing)


# ----------------------------------------------------------------------------- 16-bit operand copies
# At bf16 / fp16 matmul precision the convolutions read 16-bit copies of x and dY.  In resnet_bgru every
# conv input is a BatchNorm output and every conv dY is a BatchNorm dx (model_resnet_bgru.py:19-39), so
# BatchNorm writes the copy beside its fp32 output (srk_batchnorm_fwd16 / _bwd16, the same rounding) and
# the conv takes it instead of re-reading the fp32 tensor to round it.  The hand-over is keyed by the
# tensor's address and checked against its identity: the entry holds the fp32 tensor itself (so the
# address cannot be reused while the entry lives), its version counter (any in-place write since
# invalidates it), element count and precision.  Forward copies are made in training steps only (training
# mode, autograd on); the producing BatchNorm's backward drops its forward entry, the conv backward pops the
# dY entry it consumes, and the table is bounded (a step's worth of entries).
COPIES16 = os.environ.get("SRK_BN_COPY16", "1") != "0"   # A/B switch (tests flip it)
RELU_MASK = os.environ.get("SRK_BN_RELU_MASK", "1") != "0"   # BatchNorm ReLU bits for the backward (A/B switch)
_copies16 = {}
_COPIES16_MAX = 32   # > the live entries of one resnet_bgru / mfrn_bgru step (about 22)


def _copy16_wanted(C):
    return COPIES16 and _lib.matmul_precision() != "fp32" and C % 8 == 0


def _copy16_put(t, t16):
    _copies16.pop(t.data_ptr(), None)
    while len(_copies16) >= _COPIES16_MAX:
        _copies16.pop(next(iter(_copies16)))
    _copies16[t.data_ptr()] = (t, t._version, t.numel(), _lib.matmul_precision(), t16)


def _copy16_get(t, pop=False):
    """The producer's 16-bit copy of t (a float32 contiguous CUDA tensor) at the current precision, or None."""
    e = _copies16.get(t.data_ptr())
    if e is None:
        return None
    src, ver, n, prec, t16 = e
    ok = (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t._version == ver
          and src.data_ptr() == t.data_ptr() and prec == _lib.matmul_precision())
    if pop or not ok:
        _copies16.pop(t.data_ptr(), None)
    return t16 if ok else None


def _copy16_drop(t):
    _copies16.pop(t.data_ptr(), None)   # t is alive (saved for backward), so the entry at its address is its own


# ----------------------------------------------------------------------------- conv / pool (NHWC)
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _conv_ws(Ci, Co, KH, KW, device):
    return torch.empty(int(_lib.lib().srk_conv2d_workspace_floats(Ci, Co, KH, KW)), device=device)


def _x16_handover(x, Ci, Co, pop, w_needs_grad):
    """(x16, written) for a conv forward at 16-bit matmul precision with 8-aligned channels: the producer's 16-bit
    copy of x (written = 2: ready; popped from the table when its producer never drops it), else storage for the
    library to keep the forward's copy in when the backward will read it (the library reports in ``written``
    whether it did), else (None, 0)."""
    x16, written = None, ctypes.c_int(0)
    if _lib.matmul_precision() != "fp32" and Ci % 8 == 0 and Co % 8 == 0:
        x16 = _copy16_get(x, pop=pop)
        if x16 is not None:
            written.value = 2
        elif w_needs_grad:
            x16 = torch.empty(x.numel(), device=x.device, dtype=torch.int16)
    return x16, written


def _param_grad_target(ctx, params):
    """Where a backward may ADD the gradients of `params` (a conv's weight; BatchNorm's gamma and beta), the
    Function's inputs 1, 2, ..: their FlatParams-owned .grad buffers when every one of them has one (all or none;
    the kernel that forms the gradients then adds them in, no autograd add kernel), else None: the gradients go
    into fresh tensors and back to autograd."""
    flat = [_flat_grad(p) if ctx.needs_input_grad[1 + i] and INPLACE_GRADS else None for i, p in enumerate(params)]
    return flat if all(g is not None for g in flat) else None


def _param_grad_done(params, grads, accumulated):
    """What the backward returns for `params` after the call: None for each once accumulated in place (the gradient
    reducer is told once, with all of them), else the gradients in the parameters' shapes."""
    if not accumulated:
        return [g.view(p.shape) for g, p in zip(grads, params)]
    red = _reducer_of(params[0])
    if red is not None:
        red.mark_ready(list(params))
    return [None] * len(params)


def _dw_target(ctx, w):
    """(dw, accumulate) of a conv backward: ctx.w_param's own .grad to add into, else a fresh tensor like w."""
    flat = _param_grad_target(ctx, [ctx.w_param])
    return (flat[0], 1) if flat else (torch.empty_like(w), 0)


def _conv_operands(x, w, b):
    """x (channels last) and the weight of a dense conv forward, contiguous and checked."""
    x, w = x.contiguous(), w.contiguous()
    _check_cuda(x, w, b)
    if x.shape[-1] != w.shape[1]:
        raise _lib.SrkError("conv: input has %d channels, weight expects %d" % (x.shape[-1], w.shape[1]))
    return x, w


def _conv_forward_done(ctx, x, w, w_param, x16, written, geom):
    """What a dense conv forward leaves for its backward: w as the library saw it, w_param the parameter itself (so
    the backward can accumulate into its .grad), the 16-bit copy of x if the library kept one."""
    ctx.x16 = x16 if written.value else None
    ctx.prec = _lib.matmul_precision()
    ctx.save_for_backward(x, w)
    ctx.w_param = w_param
    ctx.geom = geom


def _conv_backward_buffers(ctx, dy, x, w, has_b, KH, KW):
    """(dy, dy16, dx, dw, accumulate, db, ws, x16) of a dense conv backward."""
    dy = dy.contiguous()
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    dw, acc = _dw_target(ctx, w)
    db = torch.empty((w.shape[0],), device=x.device) if has_b else None
    ws = _conv_ws(x.shape[-1], w.shape[0], KH, KW, x.device)
    x16 = ctx.x16 if ctx.prec == _lib.matmul_precision() else None   # a copy in this precision only
    ctx.x16 = None
    dy16 = _copy16_get(dy, pop=True)   # the producing BatchNorm backward's copy of dY
    return dy, dy16, dx, dw, acc, db, ws, x16


class _Conv2dNHWCFn(torch.autograd.Function):
    """Conv2d on channels-last [N, H, W, Ci] (srk_conv2d_nhwc_fwd16 / _bwd16_acc)."""

    @staticmethod
    def forward(ctx, x, w, b, padding, stride):
        x, wc = _conv_operands(x, w, b)
        if wc.dim() == 3:   # a Conv1d weight [Co, Ci, K] taken as [Co, Ci, 1, K]
            wc = wc.unsqueeze(2)
        N, H, W, Ci = x.shape
        Co, _, KH, KW = wc.shape
        (ph, pw), (sh, sw) = padding, stride
        y = torch.empty((N, (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1, Co), device=x.device)
        ws = _conv_ws(Ci, Co, KH, KW, x.device)
        # keep the forward's 16-bit copy of x for the backward's gathers (the library reports whether it wrote it)
        x16, written = _x16_handover(x, Ci, Co, False, ctx.needs_input_grad[1])
        call("srk_conv2d_nhwc_fwd16", ptr(x), N, H, W, Ci, ptr(wc), _optr(b), Co, KH, KW, ph, pw, sh, sw, ptr(y),
             ptr(ws), _optr(x16), ctypes.byref(written), stream_ptr())
        _conv_forward_done(ctx, x, wc, w, x16, written, (padding, stride, b is not None))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        (ph, pw), (sh, sw), has_b = ctx.geom
        N, H, W, Ci = x.shape
        Co, _, KH, KW = w.shape
        dy, dy16, dx, dw, acc, db, ws, x16 = _conv_backward_buffers(ctx, dy, x, w, has_b, KH, KW)
        call("srk_conv2d_nhwc_bwd16_acc", ptr(x), N, H, W, Ci, ptr(w), Co, KH, KW, ph, pw, sh, sw, ptr(dy),
             _optr(dy16), _optr(dx), ptr(dw), _optr(db), ptr(ws), _optr(x16), acc, stream_ptr())
        return dx, *_param_grad_done([ctx.w_param], [dw], acc), db, None, None


class Conv2d(tnn.Module):
    """nn.Conv2d-compatible parameters (weight [Co, Ci, KH, KW], bias [Co], torch init) applied to
    CHANNELS-LAST input [N, H, W, Ci] -> [N, Ho, Wo, Co] (the models keep activations NHWC)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        ref = tnn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = ref.kernel_size, ref.stride, ref.padding
        self.weight = tnn.Parameter(ref.weight.detach().clone())
        self.bias = tnn.Parameter(ref.bias.detach().clone()) if bias else None

    def forward(self, x):
        require_gpu()
        return _Conv2dNHWCFn.apply(x, self.weight, self.bias, self.padding, self.stride)


class _Conv1dDilFn(torch.autograd.Function):
    """Dilated 1-D convolution (stride 1) on channels-last [N, L, Ci] through srk_conv1d_nlc_dil_fwd / _bwd: the
    arguments, 16-bit copies and in-place weight gradient of _Conv2dNHWCFn, plus the dilation."""

    @staticmethod
    def forward(ctx, x, w, b, padding, dilation):
        x, wc = _conv_operands(x, w, b)
        N, L, Ci = x.shape
        Co, _, K = wc.shape
        y = torch.empty((N, max(L + 2 * padding - dilation * (K - 1), 0), Co), device=x.device)
        ws = _conv_ws(Ci, Co, 1, K, x.device)
        x16, written = _x16_handover(x, Ci, Co, False, ctx.needs_input_grad[1])
        call("srk_conv1d_nlc_dil_fwd", ptr(x), N, L, Ci, ptr(wc), _optr(b), Co, K, padding, dilation, ptr(y), ptr(ws),
             _optr(x16), ctypes.byref(written), stream_ptr())
        _conv_forward_done(ctx, x, wc, w, x16, written, (padding, dilation, b is not None))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        pad, dil, has_b = ctx.geom
        N, L, Ci = x.shape
        Co, _, K = w.shape
        dy, dy16, dx, dw, acc, db, ws, x16 = _conv_backward_buffers(ctx, dy, x, w, has_b, 1, K)
        call("srk_conv1d_nlc_dil_bwd", ptr(x), N, L, Ci, ptr(w), Co, K, pad, dil, ptr(dy), _optr(dy16), _optr(dx),
             ptr(dw), _optr(db), ptr(ws), _optr(x16), acc, stream_ptr())
        return dx, *_param_grad_done([ctx.w_param], [dw], acc), db, None, None


class Conv1d(tnn.Module):
    """nn.Conv1d-compatible parameters (weight [Co, Ci, K]) on channels-last input [N, L, Ci]."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, dilation=1):
        super().__init__()
        ref = tnn.Conv1d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias,
                         dilation=dilation)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = ref.kernel_size, ref.stride, ref.padding, ref.dilation
        self.weight = tnn.Parameter(ref.weight.detach().clone())
        self.bias = tnn.Parameter(ref.bias.detach().clone()) if bias else None

    def forward(self, x):
        return conv1d_nlc(x, self.weight, self.bias, self.stride[0], self.padding[0], self.dilation[0])


def conv1d_nlc(x, weight, bias=None, stride=1, padding=0, dilation=1):
    """K6 1-D convolution of channels-last [N, L, Ci] input with an nn.Conv1d weight [Co, Ci, K]; dilation > 1
    (stride 1 only) runs the dilated gathers of srk_conv1d_nlc_dil_*."""
    require_gpu()
    N, L, C = x.shape
    if dilation != 1:
        if stride != 1:
            raise _lib.SrkError("conv1d: dilation %d needs stride 1, got %d" % (dilation, stride))
        return _Conv1dDilFn.apply(x, weight, bias, int(padding), int(dilation))
    y = _Conv2dNHWCFn.apply(x.reshape(N, 1, L, C), weight, bias, (0, padding), (1, stride))
    return y.reshape(N, y.shape[2], weight.shape[0])


class _Conv1PoolFn(torch.autograd.Function):
    """conv1 + bias + MaxPool2d((1, pool)) of model_fbanks_cnn / model_spec_cnn (srk_conv1_pool_fwd /
    _wgrad / _dgrad): one input channel, the pooled NHWC output; the input gets a gradient only when it carries one
    (features behind a trainable front-end such as PCEN)."""

    @staticmethod
    def forward(ctx, x, w, b, padding, pool, y16_only=False):
        x = x.contiguous()
        _check_cuda(x, w, b)
        N, H, W = x.shape
        Co, _, KH, KW = w.shape
        y = torch.empty((N, H, W // pool, Co), device=x.device)
        arg = torch.empty((N, H, W // pool, Co), device=x.device, dtype=torch.uint8)
        # training steps in a 16-bit mode: the kernel also writes y's 16-bit operand copy, which conv2's
        # fused conv + pool takes as ready (no second pass over the fp32 activation)
        y16 = None
        if _copy16_wanted(Co) and ctx.needs_input_grad[1]:   # (forward runs under no_grad: needs_input_grad tells)
            y16 = torch.empty(y.numel(), device=x.device, dtype=torch.int16)
        # y16_only: the caller's consumer reads only the copy (fbanks_cnn's fused conv2 + pool on 16-bit operands),
        # so the library may leave the fp32 y unwritten (it does only when it writes the copy)
        written = ctypes.c_int(3 if (y16_only and y16 is not None) else 0)
        call("srk_conv1_pool_fwd16", ptr(x), N, H, W, ptr(w.contiguous()), ptr(b), Co, KH, KW, padding[0], padding[1],
             pool, ptr(y), ptr(arg), _optr(y16), ctypes.byref(written), stream_ptr())
        if written.value:
            _copy16_put(y, y16)
        ctx.save_for_backward(x, arg, w)
        ctx.geom = (Co, KH, KW, padding, pool)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, arg, w = ctx.saved_tensors
        Co, KH, KW, padding, pool = ctx.geom
        N, H, W = x.shape
        dy = dy.contiguous()
        dw = torch.empty((Co, 1, KH, KW), device=x.device)
        db = torch.empty((Co,), device=x.device)
        ws = torch.empty(int(_lib.lib().srk_conv1_pool_workspace_floats(Co, KH, KW)), device=x.device)
        call("srk_conv1_pool_wgrad", ptr(x), N, H, W, Co, KH, KW, padding[0], padding[1], pool, ptr(dy),
             ptr(arg), ptr(dw), ptr(db), ptr(ws), stream_ptr())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            call("srk_conv1_pool_dgrad", ptr(w.contiguous()), N, H, W, Co, KH, KW, padding[0], padding[1], pool,
                 ptr(dy), ptr(arg), ptr(dx), stream_ptr())
        return dx, dw, db, None, None, None


def conv1_pool(x, conv, pool, next_conv_pool16=False):
    """Fused ``pool(conv(x))`` for a one-channel NHW input when the geometry is the one
    srk_conv1_pool supports (conv1 + maxpool1 of model_fbanks_cnn / model_spec_cnn; an ``x`` that carries a
    gradient also needs a width that is a multiple of the pool's); otherwise the separate conv and pool kernels.
    Returns NHWC.
    next_conv_pool16: the result goes straight into ``conv_pool`` (fbanks_cnn conv2): in a 16-bit training
    step with 16-bit conv forwards that reads only the 16-bit copy, so the fp32 activation is not stored."""
    geom = (tuple(conv.kernel_size), tuple(conv.padding), tuple(pool.kernel_size))
    if (conv.in_channels == 1 and conv.out_channels == 64 and tuple(conv.stride) == (1, 1) and conv.bias is not None
            and geom in (((7, 3), (3, 1), (1, 3)), ((3, 7), (1, 3), (1, 5)))
            and (not x.requires_grad or x.shape[-1] % pool.kernel_size[1] == 0)):
        require_gpu()
        y16_only = bool(next_conv_pool16 and _lib.fused_conv_pool() and not _lib.option("conv_fwd_fp32"))
        return _Conv1PoolFn.apply(x, conv.weight, conv.bias, conv.padding, pool.kernel_size[1], y16_only)
    return pool(conv(x.unsqueeze(-1)))


class _ConvPoolNHWCFn(torch.autograd.Function):
    """Conv2d (stride 1) + bias + MaxPool2d((1, 4)) with the pooling in the conv's epilogue
    (srk_conv2d_nhwc_fwd_pool / _bwd_pool): conv2 + maxpool2 of model_fbanks_cnn.py:74-75,91-92.
    Only the pooled activation and a uint8 argmax are kept; the backward routes the pooled gradient
    through the argmax inside the library."""

    @staticmethod
    def forward(ctx, x, w, b, padding, pool_w):
        x = x.contiguous()
        w = w.contiguous()
        _check_cuda(x, w, b)
        N, H, W, Ci = x.shape
        Co, _, KH, KW = w.shape
        ph, pw = padding
        Ho, Wo = H + 2 * ph - KH + 1, W + 2 * pw - KW + 1
        y = torch.empty((N, Ho, Wo // pool_w, Co), device=x.device)
        arg = torch.empty((N, Ho, Wo // pool_w, Co), device=x.device, dtype=torch.uint8)
        ws = _conv_ws(Ci, Co, KH, KW, x.device)
        # the producing srk_conv1_pool_fwd16's copy is popped: nothing else drops its entry
        x16, written = _x16_handover(x, Ci, Co, True, ctx.needs_input_grad[1])
        call("srk_conv2d_nhwc_fwd_pool", ptr(x), N, H, W, Ci, ptr(w), _optr(b), Co, KH, KW, ph, pw, pool_w, ptr(y),
             ptr(arg), ptr(ws), _optr(x16), ctypes.byref(written), stream_ptr())
        ctx.x16 = x16 if written.value else None
        ctx.prec = _lib.matmul_precision()
        ctx.save_for_backward(x, w, arg)
        ctx.geom = (padding, pool_w, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, arg = ctx.saved_tensors
        (ph, pw), pool_w, has_b = ctx.geom
        N, H, W, Ci = x.shape
        Co, _, KH, KW = w.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty((Co,), device=x.device) if has_b else None
        ws = _conv_ws(Ci, Co, KH, KW, x.device)
        x16 = ctx.x16 if ctx.prec == _lib.matmul_precision() else None
        ctx.x16 = None
        call("srk_conv2d_nhwc_bwd_pool", ptr(x), N, H, W, Ci, ptr(w), Co, KH, KW, ph, pw, pool_w, ptr(dy), ptr(arg),
             _optr(dx), ptr(dw), _optr(db), ptr(ws), _optr(x16), stream_ptr())
        return dx, dw, db, None, None


def conv_pool(x, conv, pool):
    """``pool(conv(x))`` for channels-last x: one fused launch (srk_conv2d_nhwc_fwd_pool) when the
    conv has stride 1 and the pool is (1, 4) with a window count that divides the output width
    (conv2 + maxpool2 of model_fbanks_cnn); otherwise the separate conv and pool kernels."""
    kh, kw = pool.kernel_size
    KH, KW = conv.kernel_size
    ph, pw = conv.padding
    Wo = x.shape[2] + 2 * pw - KW + 1
    if (tuple(conv.stride) == (1, 1) and (kh, kw) == (1, 4) and Wo % 4 == 0 and conv.out_channels % 4 == 0
            and _lib.fused_conv_pool()):
        require_gpu()
        return _ConvPoolNHWCFn.apply(x, conv.weight, conv.bias, conv.padding, 4)
    return pool(conv(x))


class _MaxPoolNHWCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kh, kw):
        x = x.contiguous()
        _check_cuda(x)
        N, H, W, C = x.shape
        y = torch.empty((N, H // kh, W // kw, C), device=x.device)
        call("srk_maxpool_nhwc_fwd", ptr(x), N, H, W, C, kh, kw, ptr(y), stream_ptr())
        ctx.save_for_backward(x)
        ctx.k = (kh, kw)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        kh, kw = ctx.k
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        call("srk_maxpool_nhwc_bwd", ptr(x), ptr(dy.contiguous()), N, H, W, C, kh, kw, ptr(dx), stream_ptr())
        return dx, None, None


class MaxPool2d(tnn.Module):
    """nn.MaxPool2d(kernel_size) (stride = kernel, floor mode) on channels-last input."""

    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = _pair(kernel_size)

    def forward(self, x):
        return _MaxPoolNHWCFn.apply(x, self.kernel_size[0], self.kernel_size[1])


class MaxPool1d(tnn.Module):
    """nn.MaxPool1d(kernel_size) (stride = kernel) over the length axis of [N, L, C] input."""

    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size

    def forward(self, x):
        N, L, C = x.shape
        y = _MaxPoolNHWCFn.apply(x.reshape(N, L, 1, C), self.kernel_size, 1)
        return y.reshape(N, L // self.kernel_size, C)


# ----------------------------------------------------------------------------- depthwise conv / global average pool
class _DepthwiseConv2dFn(torch.autograd.Function):
    """srk_dwconv2d_nhwc_fwd / _bwd (include/srk.h): fp32 at every matmul precision, _Conv2dNHWCFn's conventions (the
    weight gradient ADDED into a FlatParams-owned .grad by the kernel that forms it, dx only when needed)."""

    @staticmethod
    def forward(ctx, x, w, b, padding, stride):
        x = x.contiguous()
        w_param = w
        w = w.contiguous()
        _check_cuda(x, w, b)
        if x.dim() != 4 or w.dim() != 4 or w.shape[0] != x.shape[3] or w.shape[1] != 1:
            raise _lib.SrkError("depthwise conv: x must be [N, H, W, C] and the weight [C, 1, KH, KW], got %s and %s"
                                % (tuple(x.shape), tuple(w.shape)))
        N, H, W, C = x.shape
        _, _, KH, KW = w.shape
        (ph, pw), (sh, sw) = padding, stride
        Ho, Wo = (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1
        y = torch.empty((N, max(Ho, 0), max(Wo, 0), C), device=x.device)
        call("srk_dwconv2d_nhwc_fwd", ptr(x), N, H, W, C, ptr(w), _optr(b), KH, KW, ph, pw, sh, sw, ptr(y),
             stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.w_param = w_param
        ctx.geom = (padding, stride, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        (ph, pw), (sh, sw), has_b = ctx.geom
        N, H, W, C = x.shape
        _, _, KH, KW = w.shape
        dy = dy.contiguous()
        _copy16_drop(dy)   # the producing BatchNorm backward's 16-bit copy of dY, which only a dense conv reads
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw, acc = _dw_target(ctx, w)
        db = torch.empty((C,), device=x.device) if has_b else None
        ws = torch.empty(int(_lib.lib().srk_dwconv2d_workspace_floats(N, H, W, C, KH, KW, ph, pw, sh, sw)),
                         device=x.device)
        call("srk_dwconv2d_nhwc_bwd", ptr(x), N, H, W, C, ptr(w), KH, KW, ph, pw, sh, sw, ptr(dy), _optr(dx), ptr(dw),
             _optr(db), ptr(ws), acc, stream_ptr())
        return dx, *_param_grad_done([ctx.w_param], [dw], acc), db, None, None


class DepthwiseConv2d(tnn.Module):
    """nn.Conv2d(C, C, kernel_size, groups=C)-compatible parameters (weight [C, 1, KH, KW], bias [C], torch init)
    applied to CHANNELS-LAST input [N, H, W, C] -> [N, Ho, Wo, C]: one filter per channel, no mixing across channels
    (srk_dwconv2d_nhwc_*: 1 <= KH, KW <= 7, strides 1 or 2, padding below the kernel size)."""

    def __init__(self, channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        ref = tnn.Conv2d(channels, channels, kernel_size, stride=stride, padding=padding, groups=channels, bias=bias)
        self.channels = channels
        self.kernel_size, self.stride, self.padding = ref.kernel_size, ref.stride, ref.padding
        self.weight = tnn.Parameter(ref.weight.detach().clone())
        self.bias = tnn.Parameter(ref.bias.detach().clone()) if bias else None

    def forward(self, x):
        require_gpu()
        return _DepthwiseConv2dFn.apply(x, self.weight, self.bias, self.padding, self.stride)


class _GlobalAvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _check_cuda(x)
        N, C = x.shape[0], x.shape[-1]
        HW = x.numel() // max(N * C, 1)
        y = torch.empty((N, C), device=x.device)
        call("srk_avgpool_nhwc_fwd", ptr(x), N, HW, C, ptr(y), stream_ptr())
        ctx.shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C = ctx.shape[0], ctx.shape[-1]
        dx = torch.empty(ctx.shape, device=dy.device)
        call("srk_avgpool_nhwc_bwd", ptr(dy.contiguous()), N, dx.numel() // (N * C), C, ptr(dx), stream_ptr())
        return dx


class GlobalAvgPool2d(tnn.Module):
    """The mean over H and W of channels-last input: [N, H, W, C] -> [N, C] (nn.AdaptiveAvgPool2d(1) + flatten)."""

    def forward(self, x):
        require_gpu()
        if x.dim() != 4:
            raise _lib.SrkError("GlobalAvgPool2d: x must be [N, H, W, C], got %s" % (tuple(x.shape),))
        return _GlobalAvgPoolFn.apply(x)


# ----------------------------------------------------------------------------- transformer encoder
class _LayerNormFn(torch.autograd.Function):
    """srk_layernorm_fwd / _bwd (include/srk.h): fp32 at every matmul precision, _BatchNormFn's conventions (dgamma /
    dbeta ADDED into FlatParams-owned .grad by the launch that forms them).  One ds serves x and the residual."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, eps):
        x = x.contiguous()
        res = None if residual is None else residual.contiguous()
        _check_cuda(x, gamma, beta, res)
        D = x.shape[-1]
        if gamma.shape != (D,) or beta.shape != (D,) or (res is not None and res.shape != x.shape):
            raise _lib.SrkError("LayerNorm: x [..., %d] needs gamma, beta [%d] and a residual of x's shape, got %s, %s, %s"
                                % (D, D, tuple(gamma.shape), tuple(beta.shape), None if res is None else tuple(res.shape)))
        M = x.numel() // max(D, 1)
        y = torch.empty_like(x)
        mean, rstd = torch.empty(M, device=x.device), torch.empty(M, device=x.device)
        call("srk_layernorm_fwd", ptr(x), _optr(res), ptr(gamma), ptr(beta), M, D, float(eps), ptr(y), ptr(mean),
             ptr(rstd), stream_ptr())
        ctx.save_for_backward(x, res, gamma, mean, rstd)
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, gamma, mean, rstd = ctx.saved_tensors
        D = x.shape[-1]
        M = x.numel() // D
        dy = dy.contiguous()
        ds = torch.empty_like(x)
        acc = _param_grad_target(ctx, ctx.params)
        dgamma, dbeta = acc if acc else (torch.empty_like(gamma), torch.empty_like(gamma))
        ws = torch.empty(int(_lib.lib().srk_layernorm_workspace_floats(M, D)), device=x.device)
        call("srk_layernorm_bwd", ptr(x), _optr(res), ptr(gamma), ptr(mean), ptr(rstd), ptr(dy), M, D, ptr(ds),
             ptr(dgamma), ptr(dbeta), 1.0 if acc else 0.0, ptr(ws), stream_ptr())
        dres = ds if res is not None and ctx.needs_input_grad[3] else None
        return (ds if ctx.needs_input_grad[0] else None, *_param_grad_done(ctx.params, (dgamma, dbeta), acc), dres,
                None)


class LayerNorm(tnn.Module):
    """``nn.LayerNorm(D)`` parameters (weight, bias; ones / zeros) over the last dimension, 1 <= D <= 1024, with an
    optional fused residual: ``forward(x, residual)`` normalises ``x + residual`` without writing the sum."""

    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        self.normalized_shape, self.eps = (int(normalized_shape),), float(eps)
        self.weight = tnn.Parameter(torch.ones(self.normalized_shape))
        self.bias = tnn.Parameter(torch.zeros(self.normalized_shape))

    def forward(self, x, residual=None):
        require_gpu()
        return _LayerNormFn.apply(x, self.weight, self.bias, residual, self.eps)


class _GELUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _check_cuda(x)
        y = torch.empty_like(x)
        call("srk_gelu_fwd", ptr(x), x.numel(), ptr(y), stream_ptr())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dx = torch.empty_like(x)
        call("srk_gelu_bwd", ptr(x), ptr(dy.contiguous()), x.numel(), ptr(dx), stream_ptr())
        return dx


class GELU(tnn.Module):
    """``nn.GELU()`` (the erf form), one kernel each way; the backward reads x."""

    def forward(self, x):
        require_gpu()
        return _GELUFn.apply(x)


class _MHSAFn(torch.autograd.Function):
    """srk_mhsa_fwd / _bwd on the packed projection qkv [B, T, 3 D] -> o [B, T, D]; fp32 at every matmul precision.
    The row log-sum-exps are all the forward keeps besides qkv."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        qkv = qkv.contiguous()
        _check_cuda(qkv)
        if qkv.dim() != 3 or qkv.shape[2] % (3 * heads):
            raise _lib.SrkError("self-attention: qkv must be [B, T, 3 * heads * dh], got %s with %d heads"
                                % (tuple(qkv.shape), heads))
        B, T, D3 = qkv.shape
        D = D3 // 3
        o = torch.empty((B, T, D), device=qkv.device)
        lse = torch.empty((B, heads, T), device=qkv.device)
        call("srk_mhsa_fwd", ptr(qkv), B, heads, T, D // heads, scale, ptr(o), ptr(lse), stream_ptr())
        ctx.save_for_backward(qkv, lse)
        ctx.consts = (heads, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, lse = ctx.saved_tensors
        heads, scale = ctx.consts
        B, T, D3 = qkv.shape
        dqkv = torch.empty_like(qkv)
        call("srk_mhsa_bwd", ptr(qkv), ptr(lse), ptr(do.contiguous()), B, heads, T, D3 // (3 * heads), scale,
             ptr(dqkv), stream_ptr())
        return dqkv, None, None


class MultiheadSelfAttention(tnn.Module):
    """``nn.MultiheadAttention(embed_dim, num_heads, batch_first=True)`` called as ``attn(x, x, x)`` without mask or
    dropout: the same parameter names, shapes and initial values (``in_proj_weight`` [3D, D], ``in_proj_bias`` [3D],
    ``out_proj``), ``forward(x [B, T, D]) -> [B, T, D]``.  The in-projection writes q, k, v packed as one [B, T, 3D]
    tensor that the attention core (srk_mhsa_*: T <= 128, head size a multiple of 4 in 4..64, scale head size ** -0.5)
    reads in place; its output is the out-projection's input, heads side by side.  The two projections are GEMMs
    and follow the matmul precision; the core is fp32."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        if embed_dim <= 0 or num_heads <= 0 or embed_dim % num_heads:
            raise ValueError("embed_dim %r must be a positive multiple of num_heads %r" % (embed_dim, num_heads))
        dh = embed_dim // num_heads
        if dh % 4 or not 4 <= dh <= 64:
            raise ValueError("head size %d is outside the attention kernel's domain (a multiple of 4 in 4..64)" % dh)
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, dh

        # torch's own initial values, drawn in torch's order (nn.MultiheadAttention: out_proj's Linear init first, then
        # xavier_uniform_ on in_proj_weight and zero biases), so one seed gives the two modules equal parameters
        self.in_proj_weight = tnn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = tnn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim)
        tnn.init.xavier_uniform_(self.in_proj_weight)
        with torch.no_grad():
            self.out_proj.bias.zero_()

    def forward(self, x):
        require_gpu()
        if x.dim() != 3 or x.shape[2] != self.embed_dim:
            raise _lib.SrkError("self-attention: x must be [B, T, %d], got %s" % (self.embed_dim, tuple(x.shape)))
        B, T, D = x.shape
        qkv = _LinearFn.apply(x.reshape(B * T, D), self.in_proj_weight, self.in_proj_bias).view(B, T, 3 * D)
        o = _MHSAFn.apply(qkv, self.num_heads, self.head_dim ** -0.5)
        return self.out_proj(o)


class TransformerEncoderLayer(tnn.Module):
    """``nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout=0, activation='gelu', batch_first=True,
    norm_first=False)``: post-norm, ``x = norm1(x + self_attn(x)); x = norm2(x + linear2(gelu(linear1(x))))``, with
    torch's submodule names, shapes and initial values, so the two ``state_dict``s are interchangeable.  Both
    residual adds run inside the LayerNorm kernels."""

    def __init__(self, d_model, nhead, dim_feedforward):
        super().__init__()
        # torch's construction order, so one seed gives torch's initial values
        self.self_attn = MultiheadSelfAttention(d_model, nhead)
        self.linear1 = Linear(d_model, dim_feedforward)
        self.linear2 = Linear(dim_feedforward, d_model)
        self.norm1 = LayerNorm(d_model)
        self.norm2 = LayerNorm(d_model)
        self.gelu = GELU()

    def forward(self, x):
        x = self.norm1(self.self_attn(x), residual=x)
        return self.norm2(self.linear2(self.gelu(self.linear1(x))), residual=x)


class _EmbedPosFn(torch.autograd.Function):
    """tokens = x W^T + b + pos for x [B T, K] and a table pos [T, N]: the table tiled over the batch is the C operand
    of the GEMM and the add is its beta = 1 epilogue (srk_gemm_f32).  The backward is _LinearFn's, plus the table's
    gradient: the column sums over the batch of dy viewed [B, T N] (srk_colsum_f32), added into a FlatParams-owned
    .grad when there is one."""

    @staticmethod
    def forward(ctx, x, w, b, pos):
        x = x.contiguous()
        _check_cuda(x, w, b, pos)
        w_param = w
        w = w.contiguous()
        M, K = x.shape
        T, N = pos.shape
        if M % T or w.shape != (N, K):
            raise _lib.SrkError("embedding: x [B * %d, K] needs a weight [%d, K], got %s and %s"
                                % (T, N, tuple(x.shape), tuple(w.shape)))
        y = pos.detach().repeat(M // T, 1)
        call("srk_gemm_f32", 0, 1, M, N, K, 1.0, ptr(x), K, ptr(w), K, 1.0, ptr(y), N, _optr(b),
             1 if b is not None else 0, stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.params = (w_param, b)
        ctx.pos = pos
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        pos = ctx.pos
        dpos = None
        if ctx.needs_input_grad[3]:
            B, n = dy.shape[0] // pos.shape[0], pos.numel()
            gp = _flat_grad(pos) if INPLACE_GRADS else None
            dpos = gp if gp is not None else torch.empty_like(pos)
            call("srk_colsum_f32", ptr(dy), B, n, n, ptr(dpos), 1.0 if gp is not None else 0.0, stream_ptr())
            if gp is not None:
                red = _reducer_of(pos)
                if red is not None:
                    red.mark_ready([pos])
                dpos = None
        return (*_LinearFn.backward(ctx, dy), dpos)


_DROPOUT_STATE = {}   # device index -> int64[2] {base seed, call counter} read by srk_dropout_fwd_state
_MASK63 = (1 << 63) - 1
_DROPOUT_REPLAY = [0]


class dropout_replay_mode:
    """Within this block eager dropout calls draw their masks as a replayed HIP graph does: from the
    device state the last seeded call left, the kernel's counter advancing per call, without
    re-deriving the seed from torch's generator.  An eager step here is then the arithmetic of a
    graph replay, mask included (tests/test_graphs_gpu.py compares the two bit for bit)."""

    def __enter__(self):
        _DROPOUT_REPLAY[0] += 1
        return self

    def __exit__(self, *exc):
        _DROPOUT_REPLAY[0] -= 1
        return False


def _dropout_state(device):
    """The device-resident dropout seed of ``device``.  Outside a graph capture it is re-derived on
    every call from torch's CUDA generator of that device — (initial seed, Philox offset), the
    offset then advanced as torch's own dropout would — folded with the data-parallel rank, so
    ``torch.manual_seed`` governs the masks (as it does the reference's nn.Dropout on the GPU) and
    the CPU generator (DataLoader shuffles, the reference's numpy/random draws) is never touched.
    Inside a capture the state is left as the last eager call set it and the kernel's own counter
    advance gives every graph replay a fresh mask."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _DROPOUT_STATE.get(idx)
    if st is None:
        st = torch.zeros(2, dtype=torch.int64, device=device)
        _DROPOUT_STATE[idx] = st
    if not torch.cuda.is_current_stream_capturing() and not _DROPOUT_REPLAY[0]:
        gen = torch.cuda.default_generators[idx]
        seed, off = gen.initial_seed(), gen.get_offset()
        gen.set_offset(off + 4)
        rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        base = ((seed * 0x9E3779B97F4A7C15) ^ (rank * 0xC2B2AE3D27D4EB4F) ^ (off << 17)) & _MASK63
        st[0].fill_(base)
        st[1].fill_(0)
    return st


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, state):
        x = x.contiguous()
        _check_cuda(x)
        y = torch.empty_like(x)
        keep = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        call("srk_dropout_fwd_state", ptr(x), x.numel(), float(p), ptr(state), ptr(y), ptr(keep), stream_ptr())
        ctx.save_for_backward(keep)
        ctx.scale = 1.0 / (1.0 - p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (keep,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("srk_dropout_apply", ptr(dy), ptr(keep), dy.numel(), float(ctx.scale), ptr(dx), stream_ptr())
        return dx, None, None


class _DropoutMaskFn(torch.autograd.Function):
    """y = x * keep / (1 - p) with a caller-supplied uint8 keep mask (srk_dropout_apply both ways)."""

    @staticmethod
    def forward(ctx, x, keep, scale):
        x = x.contiguous()
        _check_cuda(x)
        if keep.device != x.device or keep.dtype != torch.uint8 or keep.numel() != x.numel():
            raise _lib.SrkError("dropout keep mask must be a uint8 tensor of the input's size on its device")
        y = torch.empty_like(x)
        call("srk_dropout_apply", ptr(x), ptr(keep), x.numel(), float(scale), ptr(y), stream_ptr())
        ctx.save_for_backward(keep)
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        (keep,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("srk_dropout_apply", ptr(dy), ptr(keep), dy.numel(), float(ctx.scale), ptr(dx), stream_ptr())
        return dx, None, None


class Dropout(tnn.Module):
    """nn.Dropout(p=0.5): identity in eval mode; in training a Bernoulli(1-p) mask from a
    counter-based hash of a device-resident seed (``_dropout_state``: torch's CUDA generator state
    folded with the data-parallel rank, so ``torch.manual_seed`` governs the masks, ranks holding
    different clips draw independent masks, and a captured HIP graph draws a new mask per replay).

    ``set_mask(keep)`` supplies the keep mask (uint8, the input's shape) for the NEXT training
    forward instead of drawing one — how the parity tests replay a mask exported from the
    reference (tests/golden/fbanks_cnn_train_golden.npz)."""

    def __init__(self, p=0.5):
        super().__init__()
        self.p = p
        self._keep = None

    def set_mask(self, keep):
        self._keep = keep

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        if self._keep is not None:
            keep, self._keep = self._keep.to(device=x.device, dtype=torch.uint8).contiguous(), None
            if keep.shape != x.shape:
                raise ValueError("Dropout.set_mask: mask shape %s != input shape %s" % (tuple(keep.shape), tuple(x.shape)))
            return _DropoutMaskFn.apply(x, keep, 1.0 / (1.0 - self.p))
        return _DropoutFn.apply(x, self.p, _dropout_state(x.device))


# ----------------------------------------------------------------------------- batch norm
class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, training, momentum, eps, relu):
        x, M, C, y, mean, invstd, res = _bn_operands(x, gamma, beta, residual)
        y16, written = None, ctypes.c_int(0)
        if training and any(ctx.needs_input_grad[:4]) and _copy16_wanted(C):   # the consuming conv's 16-bit copy of y
            y16 = torch.empty(y.numel(), device=x.device, dtype=torch.int16)
        # the ReLU pattern as bits for the backward (1/16 of y's bytes, read twice there)
        mask = None
        if relu and RELU_MASK and any(ctx.needs_input_grad[:4]):
            mask = torch.empty(M * C // 4, device=x.device, dtype=torch.uint8)
        call("srk_batchnorm_fwd16_mask", ptr(x), M, C, ptr(gamma), ptr(beta), float(eps), float(momentum),
             int(training), ptr(running_mean), ptr(running_var), _optr(res), int(relu), ptr(y), _optr(y16),
             ctypes.byref(written), _optr(mask), ptr(mean), ptr(invstd), stream_ptr())
        if written.value:
            _copy16_put(y, y16)
        ctx.mask = mask
        ctx.save_for_backward(x, y, gamma, mean, invstd)
        ctx.params = (gamma, beta)
        ctx.flags = (int(training), int(relu), residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, invstd = ctx.saved_tensors
        training, relu, has_res = ctx.flags
        dy, M, C, dx, dres = _bn_backward_buffers(ctx, dy, x, has_res)
        _copy16_drop(y)   # the forward's copy: its consumers' backward has run
        dx16, written = None, ctypes.c_int(0)
        if dx is not None and _copy16_wanted(C):   # dx is the producing conv's dY
            dx16 = torch.empty(dx.numel(), device=x.device, dtype=torch.int16)
        # dgamma / dbeta are also ADDED to FlatParams-owned .grad buffers in the kernel that forms them
        acc = _param_grad_target(ctx, ctx.params)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        mask, ctx.mask = ctx.mask, None
        call("srk_batchnorm_bwd16_mask", ptr(x), ptr(y), _optr(mask), ptr(dy), M, C,
             ptr(gamma), ptr(mean), ptr(invstd), training, relu, _optr(dx), _optr(dx16), ctypes.byref(written),
             ptr(dgamma), ptr(dbeta), _optr(dres), ptr(acc[0]) if acc else None, ptr(acc[1]) if acc else None,
             stream_ptr())
        if written.value:
            _copy16_put(dx, dx16)
        return (dx, *_param_grad_done(ctx.params, (dgamma, dbeta), acc), dres) + (None,) * 6


# What _BatchNormFn and _SyncBatchNormFn share around their library calls.
def _bn_operands(x, gamma, beta, residual):
    """(x, M, C, y, mean, invstd, residual) of a forward: x and the residual contiguous, the operands checked, y and
    the saved statistics allocated."""
    x = x.contiguous()
    C = x.shape[-1]
    _check_cuda(x, gamma, beta, residual)
    mean, invstd = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    return x, x.numel() // C, C, torch.empty_like(x), mean, invstd, None if residual is None else residual.contiguous()


def _bn_backward_buffers(ctx, dy, x, has_res):
    """(contiguous dy, M, C, dx or None, dresidual or None) of a backward."""
    C = x.shape[-1]
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    dres = torch.empty_like(x) if has_res and ctx.needs_input_grad[3] else None
    return dy.contiguous(), x.numel() // C, C, dx, dres


class BatchNorm1d(tnn.Module):
    """nn.BatchNorm1d(C) parameters/buffers (weight, bias, running_mean, running_var,
    num_batches_tracked) on channels-last input [..., C]; optional fused residual add + ReLU."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = tnn.Parameter(torch.ones(num_features))
        self.bias = tnn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def _normalize(self, x, gamma, beta, residual, running_mean, running_var, relu):
        """The K9 call on float4-aligned channels (SyncBatchNorm1d overrides it)."""
        return _BatchNormFn.apply(x, gamma, beta, residual, running_mean, running_var, self.training, self.momentum,
                                  self.eps, relu)

    def forward(self, x, residual=None, relu=False):
        require_gpu()
        if self.num_features % 4:
            return self.forward_padded(x, residual, relu)[..., :self.num_features]
        if self.training:
            self.num_batches_tracked.add_(1)
        return self._normalize(x, self.weight, self.bias, residual, self.running_mean, self.running_var, relu)

    def forward_padded(self, x, residual=None, relu=False):
        """K9 works on float4 channel groups: a channel count that is not a multiple of 4 (the
        resnet_bgru mode-1 head's 250 / 125) runs on zero-padded channels — their statistics are
        0 / 0, their outputs beta = 0 — and the result keeps the padding ([..., C rounded up to 4],
        pad channels 0; `forward` slices it off).  ``x`` may arrive padded already.  The running
        statistics are updated on padded copies and written back."""
        require_gpu()
        if self.training:
            self.num_batches_tracked.add_(1)
        C = self.num_features
        p = (-C) % 4
        if x.shape[-1] == C + p:
            xp = x
        else:
            assert x.shape[-1] == C, (x.shape, C)
            xp = tnn.functional.pad(x, (0, p))
        rp = tnn.functional.pad(residual, (0, C + p - residual.shape[-1])) if residual is not None else None
        g = torch.cat([self.weight, self.weight.new_ones(p)])
        b = torch.cat([self.bias, self.bias.new_zeros(p)])
        rm = torch.cat([self.running_mean, self.running_mean.new_zeros(p)])
        rv = torch.cat([self.running_var, self.running_var.new_ones(p)])
        y = self._normalize(xp, g, b, rp, rm, rv, relu)
        if self.training:
            with torch.no_grad():
                self.running_mean.copy_(rm[:C])
                self.running_var.copy_(rv[:C])
        return y


# ----------------------------------------------------------------------------- synchronized batch norm
class _SyncBatchNormFn(torch.autograd.Function):
    """Training-mode BatchNorm over the GLOBAL batch of all data-parallel ranks (torch.nn.SyncBatchNorm
    semantics): this rank's (count, mean, M2) per channel are all-gathered and combined in rank order
    on the device (identical statistics on every rank); the backward all-reduces (sum g, sum g * xhat)
    for dx, while dgamma / dbeta keep this rank's contribution (the data-parallel gradient all-reduce
    sums them, as for any parameter)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, momentum, eps, relu, group):
        import torch.distributed as dist
        x, M, C, y, mean, invstd, res = _bn_operands(x, gamma, beta, residual)
        from . import parallel
        # under a HIP-graph capture the statistics exchange runs on the capture-only group, never on the
        # default group the eager warm-up steps used; the backward reuses the forward's choice
        group = parallel.group_for_now(group)
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        # all-gather as an all-reduce of rank-owned slots (x + 0 is exact; works on every backend)
        allst = torch.zeros((world, 3 * C), device=x.device)
        call("srk_batchnorm_stats", ptr(x), M, C, ptr(allst[rank]), stream_ptr())
        dist.all_reduce(allst, op=dist.ReduceOp.SUM, group=group)
        total = torch.empty(1, device=x.device)
        call("srk_batchnorm_combine", ptr(allst), world, C, float(eps), float(momentum), ptr(running_mean),
             ptr(running_var), ptr(mean), ptr(invstd), ptr(total), stream_ptr())
        call("srk_batchnorm_apply", ptr(x), M, C, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
             _optr(res), int(relu), ptr(y), stream_ptr())
        ctx.save_for_backward(x, y, gamma, mean, invstd, total)
        ctx.flags = (int(relu), residual is not None)
        ctx.group = group
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        x, y, gamma, mean, invstd, total = ctx.saved_tensors
        relu, has_res = ctx.flags
        dy, M, C, dx, dres = _bn_backward_buffers(ctx, dy, x, has_res)
        sums = torch.empty(2 * C, device=x.device)
        call("srk_batchnorm_bwd_reduce", ptr(x), ptr(y), ptr(dy), M, C, ptr(mean), ptr(invstd), relu, ptr(sums),
             stream_ptr())
        dbeta, dgamma = sums[:C].clone(), sums[C:].clone()     # this rank's contributions
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=ctx.group)
        if dx is not None or dres is not None:
            call("srk_batchnorm_bwd_dx", ptr(x), ptr(y), ptr(dy), M, C, ptr(total), ptr(gamma), ptr(mean), ptr(invstd),
                 ptr(sums), relu, _optr(dx), _optr(dres), stream_ptr())
        return (dx, dgamma, dbeta, dres) + (None,) * 6


class SyncBatchNorm1d(BatchNorm1d):
    """BatchNorm1d whose training statistics span every data-parallel rank (torch.nn.SyncBatchNorm).
    Same parameters / buffers / state_dict keys as BatchNorm1d; eval mode and a world of 1 take the
    plain BatchNorm1d path.  Build one with ``convert_sync_batchnorm(model)``."""

    # a 1-rank group normally takes the plain path; the GPU test of the captured exchange sets this
    collectives_at_world1 = False

    def __init__(self, num_features, eps=1e-5, momentum=0.1, process_group=None):
        super().__init__(num_features, eps, momentum)
        self.process_group = process_group

    def _normalize(self, x, gamma, beta, residual, running_mean, running_var, relu):
        # the padded path (channel counts not a multiple of 4: the resnet_bgru mode-1 head's 250 / 125)
        # comes through here too, so its statistics span the ranks as well
        import torch.distributed as dist
        if not (self.training and dist.is_available() and dist.is_initialized()
                and dist.get_world_size(self.process_group) > (0 if self.collectives_at_world1 else 1)):
            return super()._normalize(x, gamma, beta, residual, running_mean, running_var, relu)
        return _SyncBatchNormFn.apply(x, gamma, beta, residual, running_mean, running_var, self.momentum, self.eps,
                                      relu, self.process_group)


def convert_sync_batchnorm(module, process_group=None):
    """Replace every BatchNorm1d of ``module`` by a SyncBatchNorm1d sharing its parameters and
    buffers (torch.nn.SyncBatchNorm.convert_sync_batchnorm).  Call before FlatParams / the optimizer."""
    out = module
    if isinstance(module, BatchNorm1d) and not isinstance(module, SyncBatchNorm1d):
        out = SyncBatchNorm1d(module.num_features, module.eps, module.momentum, process_group)
        out.weight, out.bias = module.weight, module.bias
        out.running_mean, out.running_var = module.running_mean, module.running_var
        out.num_batches_tracked = module.num_batches_tracked
        out.train(module.training)
    for name, child in module.named_children():
        out.add_module(name, convert_sync_batchnorm(child, process_group))
    return out
