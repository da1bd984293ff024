"""Lattice-valued test tensors and float64 references for the special-value tests (runs no GPU code).

Tolerance tests cannot see a wrong tie-break in a max-pool window: a misrouted gradient is one element among
thousands.  The inputs here make the float64 reference and any correct kernel agree BIT FOR BIT, whatever the
summation order, so every comparison can be ``torch.equal``:

* activations and gradients are small integers ({-2..2}; {-3..3} for the one-channel image), weights are k / 8
  with |k| <= 8, biases k / 4 — all exact in bf16 and fp16, so fp32, bf16-operand and fp16-operand kernels see the
  same operands;
* every partial sum is an integer count of 1/8 units far below 2^24 (the largest, a conv1 weight gradient over
  3 x 98 x 40 windows of |dy x| <= 6, stays under 2^17 units), so fp32 accumulation is exact in any order.

The clips are built to force exact ties (``clips``): a constant clip (constant along the pooled axis W, so every
interior window ties in all positions, and the window on the left border ties WITHOUT position 0 wherever the
clipped column is the smaller), a clip with a zero-filled column band (a frequency mask) and columns alternating
between two lattice images (period 2 along W: in a width-4 window positions 0/2 tie and 1/3 tie), and a clip of
plain sparse lattice noise with few ties.  ``silent=True`` makes the constant clip all-zero (silence: the conv
output is the bias everywhere), the only constant that still ties where no window is clear of the padded border.

``conv_pool_case`` returns the inputs with the float64 references built from torch CPU ops (conv2d,
max_pool2d(return_indices=True), autograd): pooled output, first-maximum argmax byte, dx, dw and db for a
lattice-valued pooled gradient — plus the fp32 restatement and the tie census tests/test_lattice.py asserts on, so a
case that passes there cannot pass on the GPU vacuously.
"""
import functools

import torch
import torch.nn.functional as F

# N, H, W, KH, KW, pool: conv1 + maxpool1 of fbanks_cnn (7 x 3, pool 3) and spec_cnn (3 x 7, pool 5); Ci = 1, Co = 64
CONV1_CASES = [(3, 98, 120, 7, 3, 3), (2, 7, 9, 7, 3, 3), (2, 17, 13, 3, 7, 5)]
# N, H, W, Ci, Co, KH, KW, ph, pw (pool 4): fbanks_cnn conv2, the split-K forward, 3 x 3 taps on odd tile edges
CONV2_CASES = [(3, 98, 40, 64, 128, 1, 7, 0, 3), (2, 3, 8, 128, 64, 1, 7, 0, 3), (3, 5, 12, 8, 36, 3, 3, 1, 1)]
# the one shape with no window clear of the padded border (Wo = 8 under 7 taps): its constant clip is silence
SILENT = {(2, 3, 8, 128, 64, 1, 7, 0, 3)}


def conv1_key(N, H, W, KH, KW, pool):
    return (N, H, W, 1, 64, KH, KW, KH // 2, KW // 2, pool)


def conv2_key(N, H, W, Ci, Co, KH, KW, ph, pw):
    return (N, H, W, Ci, Co, KH, KW, ph, pw, 4)


def all_keys():
    return [conv1_key(*c) for c in CONV1_CASES] + [conv2_key(*c) for c in CONV2_CASES]


def lattice(shape, gen, amp=2, zeros=0.5):
    """Integers in [-amp, amp] as float32, a share ``zeros`` of them forced to 0."""
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=gen).float()
    return v * (torch.rand(tuple(shape), generator=gen) >= zeros) + 0.0   # (+ 0.0: no negative zeros)


def weights(shape, gen):
    return torch.randint(-8, 9, tuple(shape), generator=gen).float() / 8


def biases(n, gen):
    return torch.randint(-8, 9, (n,), generator=gen).float() / 4


KINDS = {2: ("constant", "noise"), 3: ("constant", "band_alt", "noise")}


def clips(N, H, W, Ci, gen, amp=2, silent=False, kinds=None):
    """[N, H, W, Ci] channels-last lattice clips, one structure per clip (module docstring); ``kinds`` defaults to
    constant / noise (N = 2), constant / band + alternating / noise (N = 3), all four and then noise (N >= 4)."""
    kinds = kinds or KINDS.get(N) or ("constant", "band", "alternating") + ("noise",) * (N - 3)
    assert len(kinds) == N
    x = lattice((N, H, W, Ci), gen, amp, zeros=0.6)
    for n, kind in enumerate(kinds):
        a, b = lattice((H, 1, Ci), gen, amp, zeros=0.25), lattice((H, 1, Ci), gen, amp, zeros=0.25)
        alt = torch.where((torch.arange(W) % 2 == 0).view(1, W, 1), a, b)
        if kind == "constant":
            x[n] = 0.0 if silent else a
        elif kind == "band":
            x[n, :, W // 4:W - W // 4] = 0.0
        elif kind == "alternating":
            x[n] = alt
        elif kind == "band_alt":
            x[n, :, :W // 2] = alt[:, :W // 2]
            x[n, :, W // 2:W // 2 + W // 3] = 0.0
        else:
            assert kind == "noise", kind
    return x


def _reference(x, w, b, gy, ph, pw, pool, dtype):
    """conv2d + bias + max_pool2d((1, pool)) and its gradients for the pooled gradient gy, in ``dtype`` on the CPU,
    channels-last in and out: (conv, y, arg, dx, dw, db); arg = position of the first maximum in each window."""
    xr = x.permute(0, 3, 1, 2).to(dtype).requires_grad_(True)
    wr, br = w.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    conv = F.conv2d(xr, wr, br, padding=(ph, pw))
    y, idx = F.max_pool2d(conv, (1, pool), return_indices=True)
    (y * gy.permute(0, 3, 1, 2).to(dtype)).sum().backward()
    Wo, Wq = conv.shape[3], y.shape[3]
    arg = (idx % Wo - pool * torch.arange(Wq)).to(torch.uint8)   # idx: flat (h, w) index of the window's maximum
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return nhwc(conv), nhwc(y), nhwc(arg), nhwc(xr.grad), wr.grad, br.grad


def tie_census(conv, KH, KW, ph, pw, H, W, pool):
    """conv: the dense float64 conv output [N, Ho, Wo, Co].  Per window: tied (its maximum occurs twice or more),
    tied_no0 (tied, and position 0 is not a maximum), interior (every position's taps clear of the padding)."""
    N, Ho, Wo, Co = conv.shape
    Wq = Wo // pool
    win = conv[:, :, :Wq * pool].reshape(N, Ho, Wq, pool, Co)
    eq = win == win.max(dim=3, keepdim=True).values
    tied = eq.sum(3) >= 2
    col_ok = (torch.arange(Wo) >= pw) & (torch.arange(Wo) + KW - 1 - pw <= W - 1)
    row_ok = (torch.arange(Ho) >= ph) & (torch.arange(Ho) + KH - 1 - ph <= H - 1)
    win_ok = col_ok[:Wq * pool].reshape(Wq, pool).all(1)
    interior = (row_ok.view(1, Ho, 1, 1) & win_ok.view(1, 1, Wq, 1)).expand(N, Ho, Wq, Co)
    return {"tied": tied, "tied_no0": tied & ~eq[:, :, :, 0], "interior": interior}


@functools.lru_cache(maxsize=None)
def conv_pool_case(N, H, W, Ci, Co, KH, KW, ph, pw, pool, kinds=None):
    """One conv + bias + max-pool case (keys: ``conv1_key`` / ``conv2_key``).  Returns a dict of CPU tensors, shared
    by every test that asks for the same key and not to be modified: float32 inputs x [N, H, W, Ci] (x[..., 0] is
    the one-channel image), w [Co, Ci, KH, KW], b [Co], gy [N, Ho, Wo // pool, Co]; the float64 references y, arg
    (uint8), dx, dw, db rounded to float32 (exactly: tests/test_lattice.py); ``ref32`` / ``ref64`` the unrounded
    tuples of both precisions and ``census`` the tie census of the float64 conv output."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * W + KH + Co)
    silent = (N, H, W, Ci, Co, KH, KW, ph, pw) in SILENT
    x = clips(N, H, W, Ci, gen, amp=3 if Ci == 1 else 2, silent=silent, kinds=kinds)
    w, b = weights((Co, Ci, KH, KW), gen), biases(Co, gen)
    Ho, Wo = H + 2 * ph - KH + 1, W + 2 * pw - KW + 1
    gy = lattice((N, Ho, Wo // pool, Co), gen, 2, zeros=0.3)
    ref64 = _reference(x, w, b, gy, ph, pw, pool, torch.float64)
    ref32 = _reference(x, w, b, gy, ph, pw, pool, torch.float32)
    case = {"x": x, "w": w, "b": b, "gy": gy, "ref32": ref32, "ref64": ref64,
            "census": tie_census(ref64[0], KH, KW, ph, pw, H, W, pool)}
    for name, t in zip(("y", "arg", "dx", "dw", "db"), ref64[1:]):
        case[name] = t if t.dtype == torch.uint8 else t.float()
    return case


@functools.lru_cache(maxsize=None)
def pool_case(N, H, W, C, kh, kw):
    """A plain max-pool case on a lattice map [N, H, W, C] (clip 0 constant along both pooled axes, the rest sparse
    noise in {-2..2}: a 98-row window holds its maximum many times over): x, gy, and float64 y, dx as float32."""
    gen = torch.Generator().manual_seed(N * 97 + H * 7 + W + kh * 3 + kw)
    x = lattice((N, H, W, C), gen, 2, zeros=0.5)
    x[0] = lattice((1, 1, C), gen, 2, zeros=0.25)
    gy = lattice((N, H // kh, W // kw, C), gen, 2, zeros=0.3)
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = F.max_pool2d(xr, (kh, kw))
    (y * gy.permute(0, 3, 1, 2).double()).sum().backward()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().float()
    return {"x": x, "gy": gy, "y": nhwc(y), "dx": nhwc(xr.grad)}


def exact16(t):
    """Every value of t survives a round trip through bf16 and through fp16."""
    return torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
