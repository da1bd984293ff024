"""SpecAugment restated (include/srk.h srk_specaug_draw / srk_specaug_apply; there is no reference counterpart, the
header's definition is the specification): the device draw in Python integers, the apply in float64 numpy.
Everything here works on the logical time-major clip [T][F]; a freq-major tensor is its transpose."""
import numpy as np

_M64 = (1 << 64) - 1


def n_params(NF, NT):
    return 2 + 2 * NF + 2 * NT


def _z(seed, i):
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(base, counter, B, T, F, W, NF, f_max, NT, t_max):
    """srk_specaug_draw's rows for the state {base, counter}: int32 [B, P]."""
    seed = (base + 0xD1B54A32D192ED03 * counter) & _M64
    P = n_params(NF, NT)
    out = np.zeros((B, P), dtype=np.int32)
    for b in range(B):
        def r(k, n):
            assert n >= 1
            return ((_z(seed, b * P + k) >> 32) * n) >> 32
        c = w = 0
        if W > 0:
            c = W + 1 + r(0, T - 2 * W - 2)
            w = c - W + r(1, 2 * W + 1)
        row = [c, w]
        for j in range(NF):
            fw = r(2 + 2 * j, f_max + 1)
            row += [r(3 + 2 * j, F - fw + 1), fw]
        for j in range(NT):
            tw = r(2 + 2 * NF + 2 * j, t_max + 1)
            row += [r(3 + 2 * NF + 2 * j, T - tw + 1), tw]
        out[b] = row
    return out


def valid_row(row, T, F, NF, NT):
    """The header's validity rule for one parameter row."""
    row = [int(v) for v in row]
    c, w = row[0], row[1]
    ok = (0 <= c <= T - 1) if c == w else (1 <= c <= T - 2 and 1 <= w <= T - 2)
    for j in range(NF):
        f0, fw = row[2 + 2 * j], row[3 + 2 * j]
        ok = ok and f0 >= 0 and fw >= 0 and f0 + fw <= F
    for j in range(NT):
        t0, tw = row[2 + 2 * NF + 2 * j], row[3 + 2 * NF + 2 * j]
        ok = ok and t0 >= 0 and tw >= 0 and t0 + tw <= T
    return ok


def warp_map(T, c, w):
    """Output frame t reads s(t) = i + a: (i int64 [T], a float64 [T]), a = (num % den) / den from the integers."""
    i = np.arange(T, dtype=np.int64)
    a = np.zeros(T, dtype=np.float64)
    if c == w:
        return i, a
    for t in range(T):
        if t <= w:
            num, den, base = t * c, w, 0
        else:
            num, den, base = (t - w) * (T - 1 - c), T - 1 - w, c
        i[t] = base + num // den
        a[t] = (num % den) / den
    return i, a


def masks(row, T, F, NF, NT):
    """(masked features bool [F], masked frames bool [T]) of one row."""
    row = [int(v) for v in row]
    fm, tm = np.zeros(F, dtype=bool), np.zeros(T, dtype=bool)
    for j in range(NF):
        fm[row[2 + 2 * j]: row[2 + 2 * j] + row[3 + 2 * j]] = True
    for j in range(NT):
        t0 = row[2 + 2 * NF + 2 * j]
        tm[t0: t0 + row[3 + 2 * NF + 2 * j]] = True
    return fm, tm


def masked_share(row, T, F, NF, NT):
    fm, tm = masks(row, T, F, NF, NT)
    return float((fm[None, :] | tm[:, None]).mean())


def apply(x, params, NF, NT, fill):
    """srk_specaug_apply on time-major clips x [B, T, F] in float64.  fill: "mean", "zero" or a number.
    Returns (y float64 [B, T, F], mask bool [B, T, F], i int64 [B, T], a float64 [B, T], fills float64 [B]);
    a clip with an invalid row is all NaN (and its mask all False)."""
    x = np.asarray(x)
    B, T, F = x.shape
    x64 = x.astype(np.float64)
    y = np.empty((B, T, F), dtype=np.float64)
    mask = np.zeros((B, T, F), dtype=bool)
    ii = np.zeros((B, T), dtype=np.int64)
    aa = np.zeros((B, T), dtype=np.float64)
    fills = np.zeros(B, dtype=np.float64)
    for b in range(B):
        row = params[b]
        if not valid_row(row, T, F, NF, NT):
            y[b] = np.nan
            fills[b] = np.nan
            continue
        fills[b] = x64[b].mean() if fill == "mean" else 0.0 if fill == "zero" else float(fill)
        i, a = warp_map(T, int(row[0]), int(row[1]))
        x0 = x64[b][i]
        x1 = x64[b][np.minimum(i + 1, T - 1)]
        warped = np.where(a[:, None] == 0, x0, x0 + a[:, None] * (x1 - x0))
        fm, tm = masks(row, T, F, NF, NT)
        mask[b] = fm[None, :] | tm[:, None]
        y[b] = np.where(mask[b], fills[b], warped)
        ii[b], aa[b] = i, a
    return y, mask, ii, aa, fills
