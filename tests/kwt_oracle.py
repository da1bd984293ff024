"""CPU statements of the attention core, LayerNorm, GELU and the fbanks_kwt plugin — TEST INFRASTRUCTURE ONLY.

``mhsa`` / ``mhsa_backward``, ``layernorm`` / ``layernorm_backward`` and ``gelu`` / ``gelu_backward`` are torch
tensor formulas in the dtype of their inputs (float64 in the tests), the backward ones written out by hand
(tests/test_kwt.py holds them to float64 autograd):

    attention, per clip b and head h, on the packed qkv [B, T, 3 H dh] (q | k | v thirds, head h the columns
    h dh .. (h + 1) dh - 1 of each):   S = scale Q K^T,  P = softmax rows,  O = P V;
        dV = P^T dO,  dP = dO V^T,  dS = P o (dP - rowsum(dO o O)),  dQ = scale dS K,  dK = scale dS^T Q
    LayerNorm over the last dimension of s = x (+ res), biased variance:
        y = xhat gamma + beta,  xhat = (s - mean) rstd;   g = dy gamma,
        ds = rstd (g - mean(g) - xhat mean(g xhat)),  dgamma = sum_m dy xhat,  dbeta = sum_m dy
    GELU (erf form):  y = x Phi(x),  dx = dy (Phi(x) + x phi(x))

``attn_case`` / ``ln_case`` are the seeded inputs with those results (rounded to float32 first: the kernels see exactly
these values), computed once and shared.  ``FbanksKwt`` is the model in torch CPU modules, built from
``torch.nn.TransformerEncoderLayer`` itself (dropout 0, gelu, batch_first, post-norm), with the plugin's ``state_dict``
keys and shapes; it runs in float64 after ``.double()``.  ``bf16_linears`` makes its Linear layers (and the attention
in- and out-projections) round their operands to bfloat16 first, the CPU emulation of ``--precision bf16``.
"""
import contextlib
import functools
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import features as OF
from oracle import models as OM


# ----------------------------------------------------------------------------- attention core
def _split(qkv, H):
    """qkv [B, T, 3 H dh] -> q, k, v [B, H, T, dh]."""
    B, T, D3 = qkv.shape
    dh = D3 // (3 * H)
    q, k, v = (t.reshape(B, T, H, dh).permute(0, 2, 1, 3) for t in qkv.split(D3 // 3, dim=2))
    return q, k, v


def _merge(t):
    """[B, H, T, dh] -> [B, T, H dh]."""
    B, H, T, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * dh)


def mhsa(qkv, H, scale):
    """-> (o [B, T, H dh], lse [B, H, T])."""
    q, k, v = _split(qkv, H)
    s = scale * (q @ k.transpose(2, 3))
    return _merge(torch.softmax(s, dim=3) @ v), torch.logsumexp(s, dim=3)


def mhsa_backward(qkv, H, scale, do):
    """dqkv [B, T, 3 H dh] of sum(o do), closed form."""
    q, k, v = _split(qkv, H)
    B, _, T, dh = q.shape
    g = do.reshape(B, T, H, dh).permute(0, 2, 1, 3)
    p = torch.softmax(scale * (q @ k.transpose(2, 3)), dim=3)
    o = p @ v
    dv = p.transpose(2, 3) @ g
    dp = g @ v.transpose(2, 3)
    ds = p * (dp - (g * o).sum(dim=3, keepdim=True))
    dq = scale * (ds @ k)
    dk = scale * (ds.transpose(2, 3) @ q)
    return torch.cat([_merge(dq), _merge(dk), _merge(dv)], dim=2)


def _seed(*vals):
    return sum(int(v) * 31 ** i for i, v in enumerate(vals)) % (1 << 32)


def _f32(t):
    return t.float().double()


@functools.lru_cache(maxsize=None)
def attn_case(B, H, T, dh, qmul):
    """Seeded float64 inputs of a case (q scaled by ``qmul``: peaky rows) with the forward and the backward."""
    g = torch.Generator().manual_seed(_seed(B, H, T, dh, qmul))
    qkv = torch.randn(B, T, 3 * H * dh, generator=g, dtype=torch.float64)
    qkv[:, :, :H * dh] *= qmul
    qkv = _f32(qkv)
    do = _f32(torch.randn(B, T, H * dh, generator=g, dtype=torch.float64))
    scale = dh ** -0.5
    o, lse = mhsa(qkv, H, scale)
    return {"qkv": qkv, "do": do, "scale": scale, "o": o, "lse": lse, "dqkv": mhsa_backward(qkv, H, scale, do)}


# ----------------------------------------------------------------------------- LayerNorm
def layernorm(x, res, gamma, beta, eps):
    """-> (y, mean [M], rstd [M]) over the last dimension of s = x (+ res)."""
    s = x if res is None else x + res
    mean = s.mean(dim=-1, keepdim=True)
    var = ((s - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (s - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_backward(x, res, gamma, eps, dy):
    """(ds, dgamma, dbeta) of sum(y dy), closed form."""
    s = x if res is None else x + res
    mean = s.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((s - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    xhat = (s - mean) * rstd
    g = dy * gamma
    ds = rstd * (g - g.mean(dim=-1, keepdim=True) - xhat * (g * xhat).mean(dim=-1, keepdim=True))
    D = x.shape[-1]
    return ds, (dy * xhat).reshape(-1, D).sum(dim=0), dy.reshape(-1, D).sum(dim=0)


LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(M, D, with_res, row_mean):
    """Seeded float64 inputs: rows of mean ``row_mean`` and spread 1 (split between x and res when there is one)."""
    g = torch.Generator().manual_seed(_seed(M, D, int(with_res), int(row_mean)))
    x = torch.randn(M, D, generator=g, dtype=torch.float64) + row_mean
    res = None
    if with_res:
        res = _f32(torch.randn(M, D, generator=g, dtype=torch.float64) * 0.5)
        x = x - res
    x = _f32(x)
    gamma = _f32(1.0 + 0.5 * torch.randn(D, generator=g, dtype=torch.float64))
    beta = _f32(torch.randn(D, generator=g, dtype=torch.float64))
    dy = _f32(torch.randn(M, D, generator=g, dtype=torch.float64))
    y, mean, rstd = layernorm(x, res, gamma, beta, LN_EPS)
    ds, dgamma, dbeta = layernorm_backward(x, res, gamma, LN_EPS, dy)
    return {"x": x, "res": res, "gamma": gamma, "beta": beta, "dy": dy, "y": y, "mean": mean, "rstd": rstd, "ds": ds,
            "dgamma": dgamma, "dbeta": dbeta}


# ----------------------------------------------------------------------------- GELU
def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _Phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def gelu(x):
    return x * _Phi(x)


def gelu_backward(x, dy):
    return dy * (_Phi(x) + x * _phi(x))


# ----------------------------------------------------------------------------- the model
_BF16 = [False]


@contextlib.contextmanager
def bf16_linears():
    """Inside: every ``F.linear`` of FbanksKwt (the torch encoder layers' included) rounds its input and weight to
    bfloat16 first, products and sums staying in the module's dtype: the arithmetic of the 16-bit-operand GEMMs."""
    real = F.linear

    def rounded(x, w, b=None):
        return real(x.bfloat16().to(x.dtype), w.bfloat16().to(w.dtype), b)

    F.linear = rounded   # nn.Linear and F.multi_head_attention_forward both look it up in torch.nn.functional
    try:
        yield
    finally:
        F.linear = real


class FbanksKwt(nn.Module):
    """models/model_fbanks_kwt.py in torch CPU modules."""

    def __init__(self, dim=64, heads=1, mlp_dim=256, layers=12):
        super().__init__()
        self.pos = nn.Parameter(torch.empty(98, dim).normal_(std=0.02))
        self.embed = nn.Linear(120, dim)
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(dim, heads, mlp_dim, dropout=0.0, activation="gelu",
                                                                batch_first=True, norm_first=False)
                                     for _ in range(layers)])
        self.fc = nn.Linear(dim, OM.NUM_CLASSES)

    @staticmethod
    def features(x):
        return torch.from_numpy(np.stack([OF.filter_banks(c) for c in x.numpy()]))

    def forward_features(self, inx):
        h = self.embed(inx.to(self.embed.weight.dtype)) + self.pos
        for layer in self.layers:
            h = layer(h)
        return self.fc(h.mean(dim=1))

    def forward(self, x):
        with torch.no_grad():
            inx = self.features(x)
        return self.forward_features(inx)
