"""Float64 CPU statement of attention pooling and of the mfcc_bgru_att plugin — TEST INFRASTRUCTURE ONLY.

    s[b,t] = scale <q[b], y[b,t]>,  alpha[b] = softmax_t(s[b]),  ctx[b] = sum_t alpha[b,t] y[b,t]

``attn_pool`` is the forward by those formulas, ``attn_pool_backward`` the closed-form gradients the kernels
implement (tests/test_attn_pool.py holds it to autograd's), ``MfccBGRUAtt`` the model: oracle.models.MfccBGRU's
features and nn.GRU, plus the query projection, the pool and fc.
"""
import torch
import torch.nn as nn

from oracle import models as OM


def attn_pool(y, q, scale):
    """y [B, T, D], q [B, D] -> (ctx [B, D], alpha [B, T]), in the dtype of y (float64 in the tests)."""
    s = scale * torch.einsum("bd,btd->bt", q, y)
    alpha = torch.softmax(s, dim=1)
    return torch.einsum("bt,btd->bd", alpha, y), alpha


def attn_pool_backward(y, q, alpha, g, scale):
    """(dy, dq) for g = dL/dctx; no gradient flows into alpha."""
    a = torch.einsum("bd,btd->bt", g, y)
    m = (alpha * a).sum(dim=1, keepdim=True)
    ds = alpha * (a - m)
    dq = scale * torch.einsum("bt,btd->bd", ds, y)
    dy = alpha.unsqueeze(2) * g.unsqueeze(1) + scale * ds.unsqueeze(2) * q.unsqueeze(1)
    return dy, dq


def pool_case(B, T, D, scale, qmul, seed=None):
    """A seeded case in float64: y uniform in [-1, 1] (a GRU output's range), q (times qmul) and dctx normal; with
    the forward and the closed-form backward."""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + D if seed is None else seed)
    y = torch.rand(B, T, D, generator=g, dtype=torch.float64) * 2 - 1
    q = torch.randn(B, D, generator=g, dtype=torch.float64) * qmul
    dctx = torch.randn(B, D, generator=g, dtype=torch.float64)
    # the kernels see float32 inputs: the reference computes in float64 on exactly those values
    y, q, dctx = (t.float().double() for t in (y, q, dctx))
    ctx, alpha = attn_pool(y, q, scale)
    dy, dq = attn_pool_backward(y, q, alpha, dctx, scale)
    return {"y": y, "q": q, "dctx": dctx, "ctx": ctx, "alpha": alpha, "dy": dy, "dq": dq}


class MfccBGRUAtt(nn.Module):
    def __init__(self, num_features=512, num_layers=2):
        super().__init__()
        self.gru = nn.GRU(39, hidden_size=num_features, num_layers=num_layers, bidirectional=True, batch_first=True)
        self.query = nn.Linear(num_features * 2, num_features * 2)
        self.fc = nn.Linear(num_features * 2, OM.NUM_CLASSES)
        self.scale = (num_features * 2) ** -0.5

    features = staticmethod(OM.MfccBGRU.features)

    def pooled(self, x):
        with torch.no_grad():
            inx = self.features(x).to(self.fc.weight.dtype)
        out, _ = self.gru(inx.transpose(1, 2))
        return attn_pool(out, self.query(out[:, -1, :]), self.scale)

    def forward(self, x):
        return self.fc(self.pooled(x)[0])

    def attention(self, x):
        with torch.no_grad():
            return self.pooled(x)[1]
