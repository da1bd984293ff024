"""Mixup and the soft-target cross-entropy restated (include/srk.h srk_mixup_draw / srk_mixup_apply /
srk_cross_entropy_mix; there is no reference counterpart, the header's definition is the specification): the device
draw in Python integers and libm doubles, the apply in numpy float32 (the kernel's own four roundings), the loss in
float64."""
import math

import numpy as np

_M64 = (1 << 64) - 1
TRIALS = 32   # SRK_MIXUP_TRIALS


def _z(seed, i):
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _u(seed, i):
    return (_z(seed, i) >> 11) * 2.0 ** -53       # exact: 53 bits times a power of two


def draw(base, counter, B, alpha):
    """srk_mixup_draw for the state {base, counter}: (lam float32 [B], partner int32 [B], trials used per clip
    int [B] (TRIALS + 1: none accepted), the smallest |S - 1| over every trial examined)."""
    seed = (base + 0xD1B54A32D192ED03 * counter) & _M64
    inv = 1.0 / alpha
    lam = np.ones(B, dtype=np.float32)
    used = np.zeros(B, dtype=np.int64)
    margin = math.inf
    if B == 1:
        return lam, np.zeros(1, dtype=np.int32), used, margin
    for b in range(B):
        used[b] = TRIALS + 1
        for k in range(TRIALS):
            i = (TRIALS * b + k) * 2
            U, V = _u(seed, i), _u(seed, i + 1)
            X, Y = (U, V) if inv == 1.0 else (math.pow(U, inv), math.pow(V, inv))
            S = X + Y
            margin = min(margin, abs(S - 1.0))
            if 0.0 < S <= 1.0:
                l = X / S
                lam[b] = np.float32(max(l, 1.0 - l))
                used[b] = k + 1
                break
    r = 1 + (((_z(seed, 64 * B) >> 32) * (B - 1)) >> 32)
    assert 1 <= r <= B - 1
    partner = ((np.arange(B, dtype=np.int64) + r) % B).astype(np.int32)
    return lam, partner, used, margin


def valid_rows(partner, lam, B):
    """The header's validity rule per row: partner in [0, B) and lam in [0, 1] (NaN is not)."""
    partner, lam = np.asarray(partner, dtype=np.int64), np.asarray(lam, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (partner >= 0) & (partner < B) & (lam >= 0) & (lam <= 1)


def apply(x, partner, lam):
    """srk_mixup_apply on x float32 [B, n]: fl(lam x_b) + fl(fl(1 - lam) x_partner), every operation float32; an
    invalid row is all NaN."""
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0]
    lam = np.asarray(lam, dtype=np.float32)
    ok = valid_rows(partner, lam, B)
    out = np.full_like(x, np.nan)
    for b in range(B):
        if ok[b]:
            l = lam[b]
            w = np.float32(1.0) - l
            out[b] = l * x[b] + w * x[int(partner[b])]      # float32 scalars times float32 arrays: no wider step
    assert out.dtype == np.float32
    return out


def soft_targets(labels, partner, lam, eps, C):
    """t[b, c] = (1 - eps) (lam_b [c == y_b] + (1 - lam_b) [c == y_partner(b)]) + eps / C, float64 [B, C].
    partner / lam None: the hard labels, smoothed."""
    labels = np.asarray(labels, dtype=np.int64)
    B = labels.shape[0]
    lam = np.ones(B) if lam is None else np.asarray(lam, dtype=np.float64)
    q = labels if partner is None else labels[np.asarray(partner, dtype=np.int64)]
    t = np.zeros((B, C), dtype=np.float64)
    t[np.arange(B), labels] += lam
    t[np.arange(B), q] += 1.0 - lam
    return (1.0 - eps) * t + eps / C


def soft_ce(logits, labels, partner, lam, eps):
    """srk_cross_entropy_mix in float64: (loss, dlogits [B, C])."""
    z = np.asarray(logits, dtype=np.float64)
    B, C = z.shape
    t = soft_targets(labels, partner, lam, eps, C)
    m = z.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
    loss = float((lse[:, 0] - (t * z).sum(axis=1)).mean())
    return loss, (np.exp(z - lse) - t) / B
