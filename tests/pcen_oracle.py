"""Float64 CPU statement of trainable PCEN and of the fbanks_cnn_pcen plugin — TEST INFRASTRUCTURE ONLY.

Per clip b, frame t, channel c, raw parameters p [4, C]:

    alpha = exp(p[0]), delta = exp(p[1]), r = exp(p[2]), s = sigmoid(p[3])
    E[t] = exp(k x[t]) (k = log_scale != 0) or x[t];  M[0] = E[0], M[t] = (1 - s) M[t-1] + s E[t]
    u = eps + M[t], g = E[t] u^-alpha, v = g + delta, y[t] = v^r - delta^r

``pcen`` is the forward by those formulas (differentiable: tests/test_pcen.py holds the closed form to its
autograd), ``pcen_backward`` the closed-form gradients the kernels implement, ``pcen_case`` the seeded inputs,
``FbanksCnnPcen`` the model: oracle.models.FbanksCNN with the front-end between its features and conv1.
All of it runs in the dtype of its inputs, so the same code gives the float32 evaluation the GPU tests scale
their bound by.
"""
import functools
import math

import numpy as np
import torch
import torch.nn as nn

from oracle import models as OM

DB_SCALE = math.log(10.0) / 20.0
EPS = 1e-6
DEFAULTS = (0.98, 2.0, 0.5, 0.025)   # alpha, delta, r, s (Wang et al. 2017)


def default_params(C, dtype=torch.float64):
    a, d, r, s = DEFAULTS
    rows = torch.tensor([math.log(a), math.log(d), math.log(r), math.log(s / (1 - s))], dtype=torch.float64)
    return rows.unsqueeze(1).repeat(1, C).to(dtype)


def constants(p):
    return p[0].exp(), p[1].exp(), p[2].exp(), torch.sigmoid(p[3])


def energy(x, log_scale):
    return torch.exp(log_scale * x) if log_scale != 0 else x


def pcen(x, p, log_scale=DB_SCALE, eps=EPS):
    """x [B, T, C], p [4, C] -> (y, M), both [B, T, C], in the dtype of x."""
    alpha, delta, r, s = constants(p)
    E = energy(x, log_scale)
    Ms = [E[:, 0]]
    for t in range(1, x.shape[1]):
        Ms.append((1 - s) * Ms[-1] + s * E[:, t])
    M = torch.stack(Ms, dim=1)
    g = E * (eps + M) ** (-alpha)
    return (g + delta) ** r - delta ** r, M


def pcen_backward(x, p, M, dy, log_scale=DB_SCALE, eps=EPS):
    """(dx [B, T, C], dp [4, C]) for dy = dL/dy, by the closed form (dp with respect to the raw parameters)."""
    alpha, delta, r, s = constants(p)
    T = x.shape[1]
    E = energy(x, log_scale)
    u = eps + M
    ua = u ** (-alpha)
    g = E * ua
    v = g + delta
    dv = dy * r * v ** (r - 1)
    d_r = (dy * (v ** r * v.log() - delta ** r * delta.log())).sum(dim=(0, 1))
    d_delta = (dv - dy * r * delta ** (r - 1)).sum(dim=(0, 1))
    d_alpha = (dv * g * (-u.log())).sum(dim=(0, 1))
    du = -alpha * dv * g / u
    G = torch.zeros_like(x)
    nxt = torch.zeros_like(x[:, 0])
    for t in range(T - 1, -1, -1):
        nxt = du[:, t] + (1 - s) * nxt
        G[:, t] = nxt
    dE = dv * ua + s * G
    dE[:, 0] = (dv * ua)[:, 0] + G[:, 0]
    d_s = (G[:, 1:] * (E[:, 1:] - M[:, :-1])).sum(dim=(0, 1))
    dx = dE * E * log_scale if log_scale != 0 else dE
    dp = torch.stack([d_alpha * alpha, d_delta * delta, d_r * r, d_s * s * (1 - s)])
    return dx, dp


# name -> (B, T, C, log_scale): the shapes tests/test_pcen_gpu.py runs, each the smallest at which a code path of
# the kernels can go wrong
CASES = {
    "1x1x1": (1, 1, 1, DB_SCALE),          # no recurrence: d_s is exactly 0
    "2x2x3": (2, 2, 3, DB_SCALE),
    "5x7x64": (5, 7, 64, DB_SCALE),
    "3x98x120": (3, 98, 120, DB_SCALE),    # the plugin's shape
    "4x130x65": (4, 130, 65, DB_SCALE),    # T past any chunk, C odd and above one wave
    "2x1024x1": (2, 1024, 1, DB_SCALE),
    "1x3x1024": (1, 3, 1024, DB_SCALE),
    "3x9x5lin": (3, 9, 5, 0.0),            # linear mode
    "6x98x120": (6, 98, 120, DB_SCALE),    # CPU only: the closed form against autograd
}


@functools.lru_cache(maxsize=None)
def pcen_case(name):
    """The seeded float64 inputs of a case with the forward and the closed-form backward (computed once, shared,
    never written to).  dB cases draw x from U[20, 220] and splice in, as far as B and T allow, a loud-then-silent
    clip (clip 0), a silent one (clip 1; every band at 20 log10(eps_f64)) and a silent-then-loud one (clip 2), so
    some loud frames always remain to set the scale of the comparison; linear cases draw
    lognormal energies with one exact 0.  Raw parameters: the defaults plus N(0, 0.3^2) per channel.  Every input
    is rounded to float32 first: the kernels see exactly these values."""
    B, T, C, log_scale = CASES[name]
    g = torch.Generator().manual_seed(7000 + 100 * B + 10 * T + C)
    if log_scale != 0:
        x = 20.0 + 200.0 * torch.rand(B, T, C, generator=g, dtype=torch.float64)
        silent = 20.0 * math.log10(np.finfo(np.float64).eps)
        h = T // 2
        if T > 1:
            x[0, h:] = silent       # loud, then silent
        if B > 1:
            x[1] = silent
        if B > 2:
            x[2, :h] = silent       # silent, then loud
    else:
        x = torch.exp(2.0 * torch.randn(B, T, C, generator=g, dtype=torch.float64))
        x[0, T // 2, 0] = 0.0
    p = default_params(C) + 0.3 * torch.randn(4, C, generator=g, dtype=torch.float64)
    dy = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    x, p, dy = (t.float().double() for t in (x, p, dy))
    y, M = pcen(x, p, log_scale)
    dx, dp = pcen_backward(x, p, M, dy, log_scale)
    return {"x": x, "p": p, "dy": dy, "y": y, "M": M, "dx": dx, "dp": dp, "log_scale": log_scale, "eps": EPS}


@functools.lru_cache(maxsize=None)
def pcen_case_f32(name):
    """The same statement evaluated in float32 on the CPU: its distance to float64 scales the kernels' bound."""
    c = pcen_case(name)
    x, p, dy = (c[k].float() for k in ("x", "p", "dy"))
    y, M = pcen(x, p, c["log_scale"])
    dx, dp = pcen_backward(x, p, M, dy, c["log_scale"])
    return {"y": y, "M": M, "dx": dx, "dp": dp}


def max_err(out, ref):
    """max |out - ref| / max |ref| over every element (absolute when the reference is all zero)."""
    out, ref = out.double(), ref.double()
    scale = float(ref.abs().max())
    return float((out - ref).abs().max()) / (scale if scale > 0 else 1.0)


def row_err(out, ref):
    """dp [4, C]: per row ||out - ref||_2 / ||ref||_2 (absolute where the reference row is all zero), the worst."""
    out, ref = out.double(), ref.double()
    n = ref.norm(dim=1)
    return float(((out - ref).norm(dim=1) / torch.where(n > 0, n, torch.ones_like(n))).max())


def errors(out, ref):
    """{"y", "M", "dx", "dp"} errors of a result dict against a reference one."""
    return {"y": max_err(out["y"], ref["y"]), "M": max_err(out["M"], ref["M"]), "dx": max_err(out["dx"], ref["dx"]),
            "dp": row_err(out["dp"], ref["dp"])}


class FbanksCnnPcen(OM.FbanksCNN):
    """oracle.models.FbanksCNN with PCEN applied to its [B, 98, 120] dB features before conv1; ``pcen.params``
    [4, 120] is the one new state_dict key."""

    class _Pcen(nn.Module):
        def __init__(self, C):
            super().__init__()
            self.params = nn.Parameter(default_params(C, torch.float32))

        def forward(self, x):
            return pcen(x, self.params)[0]

        def constants(self):
            with torch.no_grad():
                return dict(zip(("alpha", "delta", "r", "s"), constants(self.params.detach())))

    def __init__(self):
        super().__init__()
        self.pcen = self._Pcen(120)

    def forward_features(self, inx):
        return super().forward_features(self.pcen(inx.to(self.pcen.params.dtype)))
