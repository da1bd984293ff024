"""float64 restatement of the extended optimizer step (srk_adamw_step, optim.Adam): the global gradient norm, the clip
coefficient, masked decoupled decay, Adam, the weight EMA and the loss scaler's skip.  numpy only.

tests/test_optim_ext.py holds it to CPU torch (clip_grad_norm_ + AdamW) in float64; the GPU tests compare the kernels
against it.
"""
import numpy as np

CHUNK = 64      # floats per decay-mask byte


def grad_norm(g, s=1.0):
    """sqrt(sum (g * s)^2) over the flat gradient, the scale applied before squaring."""
    g = np.asarray(g, dtype=np.float64) * float(s)
    return float(np.sqrt(np.sum(g * g)))


def clip_coef(total_norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (total_norm + 1e-6)); 1 with clipping off."""
    if max_norm is None or max_norm <= 0 or np.isinf(max_norm):
        return 1.0
    return min(1.0, float(max_norm) / (total_norm + 1e-6))


def expand_mask(mask, n):
    """The per-element decay flags of a chunk mask (None = decay everything)."""
    if mask is None:
        return np.ones(n, dtype=bool)
    return np.repeat(np.asarray(mask).astype(bool), CHUNK)[:n]


class State:
    def __init__(self, p, ema=False):
        self.p = np.array(p, dtype=np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.ema = self.p.copy() if ema else None
        self.step = 0
        self.clipped_steps = 0
        self.overflows = 0
        self.total_norm = 0.0
        self.coef = 1.0


def step(st, g, lr, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, loss_scale=None, weight_decay=0.0, mask=None,
         max_norm=None, ema_decay=None):
    """One step on `st` in place.  loss_scale: the scaler's scale (the gradient is divided by it); a non-finite
    gradient element then skips the step: nothing but the overflow count changes."""
    g = np.asarray(g, dtype=np.float64)
    s = grad_scale if loss_scale is None else grad_scale / loss_scale
    if loss_scale is not None and not np.isfinite(g).all():
        st.overflows += 1
        return st
    st.total_norm = grad_norm(g, s)
    st.coef = clip_coef(st.total_norm, max_norm)
    if st.coef < 1.0:
        st.clipped_steps += 1
    st.step += 1
    b1, b2 = betas
    gg = g * s * st.coef
    if weight_decay:
        st.p = np.where(expand_mask(mask, g.size), st.p * (1.0 - lr * weight_decay), st.p)
    st.m = b1 * st.m + (1.0 - b1) * gg
    st.v = b2 * st.v + (1.0 - b2) * gg * gg
    denom = np.sqrt(st.v) / np.sqrt(1.0 - b2 ** st.step) + eps
    st.p = st.p - (lr / (1.0 - b1 ** st.step)) * (st.m / denom)
    if st.ema is not None:
        st.ema = ema_decay * st.ema + (1.0 - ema_decay) * st.p
    return st
