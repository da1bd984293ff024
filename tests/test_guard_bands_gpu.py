"""Guard bands around every buffer a C-ABI entry point is given (tests/guarded.py).

Each case runs the same calls three times: on ordinary, generously sized tensors (the plain run), and twice with
every pointer argument — inputs, outputs, state words, workspaces — between two 64 KiB bands, the caller-sized
workspaces exactly as large as their srk_*_workspace_* query says and pre-filled with zeros in one run and with
0xFF bytes (NaN) in the other.  Asserted: every band intact and no const input modified (after every call: a
forward workspace is checked again after the backward), every floating-point output finite, every output the plain
run's bits (the kernels are documented as deterministic; a read past an input's end picks up NaN), no output
element left unwritten where the header says it is written, and the same bits whatever the workspace held.

The dense cases are also held to the float64 product with padded leading dimensions.
"""
import contextlib
import ctypes
import math

import pytest
import torch

from guarded import Arena, band_value, same_bits
from speechrecognitionproject_amd import _lib

pytestmark = pytest.mark.gpu

F32, I64, I32, I16, U8, F64 = torch.float32, torch.int64, torch.int32, torch.int16, torch.uint8, torch.float64
DT16 = {"bf16": torch.bfloat16, "fp16": torch.float16}

# ----------------------------------------------------------------------------- the case table
# Dense: entry, options, precision, ta, tb, M, N, K, lead, bias_mode — the rows of test_dense_gpu.py's
# test_gemm_runs_what_the_plan_describes (every kernel family below 300 x 260 x 1024), run with lda = width + 8,
# ldb = width + 8, ldc = N + 4; beta = 1.5 on every other row; lead = 1: A and C one element off 16 bytes.
_GEMM_ROWS = [
    ("f32", {}, "fp32", 0, 1, 256, 12, 1024, 0, 1),              # skinny_n
    ("f32", {}, "bf16", 1, 0, 12, 260, 300, 0, 0),               # skinny_m
    ("f32", {}, "fp16", 0, 0, 300, 260, 16, 0, 2),               # skinny_k
    ("f32", {"gemm_skinny": 0}, "fp32", 0, 0, 300, 12, 1024, 0, 0),   # the tile path instead
    ("f32", {}, "fp32", 0, 0, 300, 260, 1024, 0, 1),             # 64 x 64, split K, vector reduce
    ("f32", {}, "fp32", 0, 1, 300, 260, 1024, 0, 0),             # x W^T: 4 waves
    ("f32", {}, "fp32", 1, 0, 300, 259, 1023, 0, 2),             # scalar staging, scalar reduce
    ("f32", {}, "fp32", 1, 1, 37, 29, 39, 1, 0),                 # operand one element off 16 B
    ("f32", {}, "fp32", 0, 0, 65, 65, 17, 0, 0),                 # unsplit
    ("rowsum", {}, "fp32", 1, 0, 96, 64, 1024, 0, 0),            # split K with row-sum partials
    ("f32", {"gemm32_kernel": 2}, "fp32", 0, 0, 300, 260, 1024, 0, 1),   # ping-pong, split
    ("f32", {"gemm32_kernel": 2}, "fp32", 1, 1, 256, 256, 64, 0, 0),
    ("rowsum", {"gemm32_kernel": 2}, "fp32", 1, 0, 300, 260, 1024, 0, 0),
    ("f32", {"gemm32_kernel": 2}, "fp32", 0, 0, 300, 260, 1024, 1, 0),   # ... refused by alignment: tile kernel
    ("f32", {}, "bf16", 0, 0, 300, 260, 1024, 0, 1),             # gemm_lp_kernel, vector staging
    ("f32", {}, "fp16", 0, 1, 299, 260, 1023, 0, 2),             # gemm_lp_kernel, scalar staging
    ("rowsum", {}, "bf16", 1, 0, 300, 260, 1024, 0, 0),
    ("g16", {}, "bf16", 0, 0, 296, 256, 1024, 0, 1),             # gemm_h16_kernel
    ("g16", {}, "fp16", 1, 0, 296, 256, 1024, 0, 0),
    ("g16", {"gemm16_kernel": 2}, "bf16", 0, 1, 296, 256, 1024, 0, 2),   # gemm_g16_kernel
    ("g16b", {}, "fp16", 0, 0, 296, 256, 1024, 0, 0),            # batched: gemm_g16_kernel
]
# the fp32 rows once more with lead = 1
_GEMM_ROWS += [r[:8] + (1, r[9]) for r in _GEMM_ROWS if r[2] == "fp32" and r[8] == 0]
GEMM = [pytest.param(*r, 1.5 if i % 2 else 0.0, id="%s-%s-%d%d-%dx%dx%d-lead%d-%d" % (r[0], r[2], r[3], r[4], r[5], r[6],
                                                                                   r[7], r[8], i))
        for i, r in enumerate(_GEMM_ROWS)]
# M, N, ldx, beta, lead  (builder's choice: one past the 4-wide vector / the 256-column block; ldx > N)
COLSUM = [(37, 29, 33, 0.0, 0), (300, 257, 261, 1.5, 0), (37, 29, 33, 1.5, 1)]

# GRU: precision, B, T, in, H
GRU = [("fp32", 5, 3, 39, 128),      # in % 4 != 0: the padded-input blocks
       ("fp32", 33, 2, 20, 256),
       ("fp32", 3, 2, 20, 512),      # the fused input projection
       ("fp32", 70, 2, 72, 512),     # in > 64, B no multiple of 64
       ("bf16", 70, 2, 39, 512), ("fp16", 70, 2, 39, 512),      # in8 != in: the dxpad8 block
       ("bf16", 300, 2, 24, 512), ("fp16", 300, 2, 24, 512),    # more than 256 rows
       # builder's choice: T one past the persistent kernels' 3-slot hand-off ring plus its first step (the slot
       # index wraps), and the fp32 kernels' second 256-row launch
       ("fp32", 70, 5, 72, 512), ("bf16", 70, 5, 39, 512), ("fp32", 300, 2, 24, 512)]
GRU_X16 = [("bf16", 5, 3, 24, 512), ("fp16", 5, 3, 24, 512)]    # builder's choice: the smallest two-layer call
GRU_TOP_LAST = [0, 2, 3]                                        # option gru_top_last at (5, 3, 1024, 512)

# Conv: N, H, W, Ci, Co, KH, KW, ph, pw, sh, sw
CONV = [(2, 9, 11, 5, 7, 3, 2, 1, 0, 1, 1),
        (4, 17, 13, 12, 36, 3, 3, 1, 1, 2, 2),
        (2, 5, 7, 8, 24, 3, 3, 1, 1, 1, 1),
        (2, 1, 125, 64, 128, 1, 15, 0, 7, 1, 2),
        (2, 3, 10, 128, 256, 1, 10, 0, 0, 1, 1)]   # full width: the forward is a plain GEMM
CONV_RING = (2, 98, 40, 64, 128, 1, 7, 0, 3, 1, 1)   # under conv_ring = 0x87 and the default; also the pooled pair
# builder's choice: the smallest batch of that layer that the 256-row fp32 conv tiles (option conv_tile = 256) take:
# 66640 output rows = 260 tiles and a partial one
CONV_TILE256 = (17, 98, 40, 64, 128, 1, 7, 0, 3, 1, 1)
CONV_16 = (2, 5, 7, 8, 24, 3, 3, 1, 1, 1, 1)         # fwd16 / bwd16 / bwd16_dy16 / bwd16_acc
CONV1D_DIL = (2, 37, 16, 32, 5, 8, 4)                # N, L, Ci, Co, K, pad, dil
CONV1_POOL = [(2, 7, 9, 7, 3, 3), (2, 4, 13, 3, 7, 5)]   # N, H, W, KH, KW, pool
MAXPOOL = [(2, 5, 7, 4, 2, 3)]                       # N, H, W, C, kh, kw

BN = [(7, 4), (750, 256), (508, 252)]                # M, C  ((750, 256): several chunks)
CE = [(5, 12, 0), (9, 130, 0), (5, 12, 1)]           # B, C, lead
ADAM_N = [1, 5, 1027, 2099201]                       # the last: past one grid stride of 2048 x 256 x 4
DROPOUT = [(1, 0), (255, 0), (1025, 0), (255, 1)]    # n, lead
ENSEMBLE = [(3, 5, 12, 0), (8, 257, 64, 0), (3, 5, 12, 1)]   # K, B, C, lead

ATTN = [(3, 5, 12, 0), (2, 65, 10, 0), (2, 64, 1024, 0), (3, 5, 12, 1)]   # B, T, D, lead
PCEN = [(2, 3, 5), (3, 98, 120)]                     # B, T, C
DWCONV = [(2, 5, 7, 6, 3, 3, 1, 1, 2, 2, 0),         # N, H, W, C, KH, KW, ph, pw, sh, sw, lead; scalar path
          (2, 9, 8, 8, 3, 3, 1, 1, 1, 2, 0),
          (2, 9, 8, 8, 3, 3, 1, 1, 1, 2, 1)]
AVGPOOL = [(3, 7, 6)]                                # N, HW, C
SPECAUG = [(51, 39), (98, 40)]                       # T, F  (51 x 39: the scalar path)


# ----------------------------------------------------------------------------- the three runs of a case
class Outs:
    """What one run of a case produced: (name, tensor, every element written by the call?)."""

    def __init__(self):
        self.items = []

    def add(self, name, t, written=True):
        self.items.append((name, t.detach().clone(), written))


def _never_written(t):
    """Elements of an output that still hold the pattern an "out" buffer is pre-filled with."""
    iv, pat = band_value(t.dtype, "out")
    return int((t.contiguous().reshape(-1).view(iv) == pat).sum())


def run_case(fn):
    """fn(arena, outs) makes the case's calls.  Returns the plain run's outputs {name: tensor}."""
    runs = []
    for guarded, ws_byte in ((False, 0x00), (True, 0x00), (True, 0xFF)):
        a, o = Arena(guarded, ws_byte), Outs()
        fn(a, o)
        a.check()
        runs.append(o)
    plain = runs[0]
    for what, run in (("plain", plain), ("guarded, zeroed workspace", runs[1]), ("guarded, 0xFF workspace", runs[2])):
        assert [i[0] for i in run.items] == [i[0] for i in plain.items]
        for (name, ref, written), (_, t, _) in zip(plain.items, run.items):
            if t.dtype.is_floating_point:
                assert bool(torch.isfinite(t.float() if t.dtype != F64 else t).all()), "%s: non-finite (%s)" % (name, what)
            if written:
                assert _never_written(t) == 0, "%s: %d elements never written (%s)" % (name, _never_written(t), what)
            assert same_bits(ref, t), "%s: differs from the plain run (%s)" % (name, what)
    return {name: t for name, t, _ in plain.items}


@contextlib.contextmanager
def precision(prec, **opts):
    try:
        _lib.set_matmul_precision(prec)
        with _lib.options(**opts):
            yield
    finally:
        _lib.set_matmul_precision("fp32")


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) + 1)


def _rn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _ws_floats(name, *dims):
    return int(getattr(_lib.lib(), name)(*dims))


def _flag():
    return ctypes.c_int(0)


# ----------------------------------------------------------------------------- dense
def _mat_mask(n, batch, rows, cols, ld, stride):
    """Which of the n elements of a buffer belong to `batch` matrices [rows][cols] at leading dimension ld,
    `stride` elements apart."""
    i = torch.arange(n)
    z, r = (i // stride, i % stride) if batch > 1 else (torch.zeros_like(i), i)
    return ((z < batch) & (r // ld < rows) & (r % ld < cols)).cuda()


def _padded(vals, ld, stride, dtype):
    """vals [batch][rows][cols] laid out at leading dimension ld / batch stride `stride`, NaN in every gap; exactly
    as long as the last element requires."""
    batch, rows, cols = vals.shape
    n = (batch - 1) * stride + (rows - 1) * ld + cols
    flat = torch.full((n,), float("nan"), dtype=dtype, device="cuda")
    flat[_mat_mask(n, batch, rows, cols, ld, stride)] = vals.to(dtype).reshape(-1)
    return flat


@pytest.mark.parametrize("entry,opts,prec,ta,tb,M,N,K,lead,bias,beta", GEMM)
def test_gemm(gpu, entry, opts, prec, ta, tb, M, N, K, lead, bias, beta):
    o16, batch = entry in ("g16", "g16b"), 2 if entry == "g16b" else 1
    ar, ac = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    lda, ldb, ldc = ac + 8, bc + 8, N + 4
    sA, sB, sC = ar * lda + 8, br * ldb + 16, M * ldc + 4     # used by the batched entry only
    g = _gen(M, N, K, ta, tb, lead)
    dt = DT16[prec] if o16 else F32
    A = torch.randn(batch, ar, ac, generator=g).to(dt).cuda()
    B = torch.randn(batch, br, bc, generator=g).to(dt).cuda()
    C0 = torch.randn(batch, M, N, generator=g).cuda()
    bv = torch.randn(M if bias == 2 else N, generator=g).cuda()
    rs0 = torch.randn(M, generator=g).cuda()
    alpha = 0.5
    nC = (batch - 1) * sC + (M - 1) * ldc + N
    cmask = _mat_mask(nC, batch, M, N, ldc, sC)

    def fn(a, o):
        Ab = a.inp("A", _padded(A, lda, sA, dt), lead=lead)
        Bb = a.inp("B", _padded(B, ldb, sB, dt))
        Cb = a.out("C", nC, F32, lead=lead)
        if beta != 0.0:
            Cb.t[cmask] = C0.reshape(-1)
        bb = a.inp("bias", bv) if bias else None
        if entry == "rowsum":
            rb = a.out("rowsum", M, F32, init=rs0 if beta != 0.0 else None)
            a.call("srk_gemm_rowsum_f32", ta, tb, M, N, K, alpha, Ab, lda, Bb, ldb, beta, Cb, ldc, rb)
            o.add("rowsum", rb.t)
        elif entry == "g16b":
            a.call("srk_gemm_16_batched", ta, tb, M, N, K, alpha, Ab, lda, sA, Bb, ldb, sB, beta, Cb, ldc, sC, batch)
        else:
            a.call("srk_gemm_16" if o16 else "srk_gemm_f32", ta, tb, M, N, K, alpha, Ab, lda, Bb, ldb, beta, Cb, ldc,
                   bb, bias)
        # the gaps between C's rows (and matrices) still hold the "out" pattern
        assert _never_written(Cb.t[~cmask]) == int((~cmask).sum()), "C: a gap between rows was written"
        o.add("C", Cb.t[cmask])

    with precision(prec, **opts):
        got = run_case(fn)
    # values: fp32 accumulation over K terms, in 16-bit modes both operands rounded to at worst bf16
    opA, opB = A.float().cpu().double(), B.float().cpu().double()
    opA, opB = (opA.transpose(1, 2) if ta else opA), (opB.transpose(1, 2) if tb else opB)
    ref = alpha * (opA @ opB) + beta * C0.cpu().double()
    if bias:
        ref += bv.cpu().double() if bias == 1 else bv.cpu().double()[:, None]
    eps = K * 2.0 ** -23 + (2.0 ** -7 if prec != "fp32" else 0.0)
    bound = eps * alpha * float((opA.abs() @ opB.abs()).max()) + 1e-6
    if beta != 0.0:
        bound += float((beta * C0).abs().max()) * 2.0 ** -23
    err = float((got["C"].cpu().double().view(batch, M, N) - ref).abs().max())
    assert err <= bound, (err, bound)
    if entry == "rowsum":   # the fused sums are over the UNROUNDED op(A)
        rref = opA[0].sum(1) + beta * rs0.cpu().double()
        rb = K * 2.0 ** -23 * float(opA[0].abs().sum(1).max()) + 1e-6 + float((beta * rs0).abs().max()) * 2.0 ** -23
        assert float((got["rowsum"].cpu().double() - rref).abs().max()) <= rb


@pytest.mark.parametrize("M,N,ldx,beta,lead", COLSUM)
def test_colsum(gpu, M, N, ldx, beta, lead):
    g = _gen(M, N, ldx)
    X = torch.randn(1, M, N, generator=g).cuda()
    out0 = torch.randn(N, generator=g).cuda()

    def fn(a, o):
        xb = a.inp("X", _padded(X, ldx, 0, F32), lead=lead)
        ob = a.out("out", N, F32, init=out0 if beta != 0.0 else None, lead=lead)
        a.call("srk_colsum_f32", xb, M, N, ldx, ob, beta)
        o.add("out", ob.t)

    got = run_case(fn)
    ref = X[0].cpu().double().sum(0) + beta * out0.cpu().double()
    bound = (M + 1) * 2.0 ** -23 * float((X[0].abs().sum(0) + abs(beta) * out0.abs()).max()) + 1e-6
    assert float((got["out"].cpu().double() - ref).abs().max()) <= bound


# ----------------------------------------------------------------------------- GRU
def _gru_weights(g, IN, H):
    k = 1.0 / math.sqrt(H)
    return [_rn(g, 2, 3 * H, IN, scale=k), _rn(g, 2, 3 * H, H, scale=k), _rn(g, 2, 3 * H, scale=k),
            _rn(g, 2, 3 * H, scale=k)]


def _gru_grads(a, g, IN, H, accumulate, tag=""):
    shapes = [(2, 3 * H, IN), (2, 3 * H, H), (2, 3 * H), (2, 3 * H)]
    inits = [_rn(g, *s, scale=0.1) if accumulate else None for s in shapes]
    return [a.out(tag + n, math.prod(s), F32, init=i)
            for n, s, i in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), shapes, inits)]


@pytest.mark.parametrize("accumulate,with_dx", [(0, True), (1, False)])
@pytest.mark.parametrize("prec,B,T,IN,H", GRU)
def test_gru_layer(gpu, prec, B, T, IN, H, accumulate, with_dx):
    def fn(a, o):
        g = _gen(B, T, IN, H)
        x = a.inp("x", _rn(g, B, T, IN))
        w = [a.inp(n, t) for n, t in zip(("w_ih", "w_hh", "b_ih", "b_hh"), _gru_weights(g, IN, H))]
        y = a.out("y", B * T * 2 * H)
        ws = a.ws("ws_fwd", _ws_floats("srk_gru_workspace_floats", B, T, IN, H, 0))
        a.call("srk_gru_layer_fwd", x, B, T, IN, H, *w, y, ws)
        o.add("y", y.t)
        dy = a.inp("dy", _rn(g, B, T, 2 * H))
        dx = a.out("dx", B * T * IN) if with_dx else None
        grads = _gru_grads(a, g, IN, H, accumulate)
        ws2 = a.ws("ws_bwd", _ws_floats("srk_gru_workspace_floats", B, T, IN, H, 1))
        a.call("srk_gru_layer_bwd", x, B, T, IN, H, w[0], w[1], y, ws, dy, dx, *grads, accumulate, ws2)
        for n, b in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), [dx] + grads):
            if b is not None:
                o.add(n, b.t)

    with precision(prec):
        run_case(fn)
    assert _lib.spin_timeouts() == 0


@pytest.mark.parametrize("prec,B,T,IN,H", GRU_X16)
def test_gru_two_layers_x16(gpu, prec, B, T, IN, H):
    """Layer 2 reads layer 1's own 16-bit copy of y inside layer 1's (guarded) forward workspace."""
    def fn(a, o):
        g = _gen(B, T, IN, H, 16)
        x = a.inp("x", _rn(g, B, T, IN))
        w1 = [a.inp("l1." + n, t) for n, t in zip(("w_ih", "w_hh", "b_ih", "b_hh"), _gru_weights(g, IN, H))]
        y1 = a.out("y1", B * T * 2 * H)
        n1 = _ws_floats("srk_gru_workspace_floats", B, T, IN, H, 0)
        ws1 = a.ws("l1.ws_fwd", n1)
        a.call("srk_gru_layer_fwd_x16", x, None, B, T, IN, H, *w1, y1, ws1)
        off = _ws_floats("srk_gru_y16_offset", B, T, IN, H)
        assert 0 <= off and off * 4 + B * T * 2 * H * 2 <= n1 * 4, "y16 lies outside the forward workspace"
        y16 = ctypes.c_void_p(ws1.data_ptr() + 4 * off)
        IN2 = 2 * H
        w2 = [a.inp("l2." + n, t) for n, t in zip(("w_ih", "w_hh", "b_ih", "b_hh"), _gru_weights(g, IN2, H))]
        y2 = a.out("y2", B * T * 2 * H)
        ws2 = a.ws("l2.ws_fwd", _ws_floats("srk_gru_workspace_floats", B, T, IN2, H, 0))
        a.call("srk_gru_layer_fwd_x16", y1, y16, B, T, IN2, H, *w2, y2, ws2)
        o.add("y1", y1.t)
        o.add("y2", y2.t)
        dy2 = a.inp("dy2", _rn(g, B, T, 2 * H))
        dy1 = a.out("dy1", B * T * IN2)
        g2 = _gru_grads(a, g, IN2, H, 0, "l2.")
        wsb2 = a.ws("l2.ws_bwd", _ws_floats("srk_gru_workspace_floats", B, T, IN2, H, 1))
        a.call("srk_gru_layer_bwd_x16", y1, y16, B, T, IN2, H, w2[0], w2[1], y2, ws2, dy2, dy1, *g2, 0, wsb2)
        dx = a.out("dx", B * T * IN)
        g1 = _gru_grads(a, g, IN, H, 0, "l1.")
        wsb1 = a.ws("l1.ws_bwd", _ws_floats("srk_gru_workspace_floats", B, T, IN, H, 1))
        a.call("srk_gru_layer_bwd_x16", x, None, B, T, IN, H, w1[0], w1[1], y1, ws1, dy1, dx, *g1, 0, wsb1)
        for n, b in zip(("dy1", "dx", "l2.dw_ih", "l2.dw_hh", "l2.db_ih", "l2.db_hh", "l1.dw_ih", "l1.dw_hh", "l1.db_ih",
                         "l1.db_hh"), [dy1, dx] + g2 + g1):
            o.add(n, b.t)

    with precision(prec):
        run_case(fn)
    assert _lib.spin_timeouts() == 0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("top_last", GRU_TOP_LAST)
def test_gru_top_last(gpu, top_last, accumulate):
    B, T, IN, H = 5, 3, 1024, 512
    modes = []

    def fn(a, o):
        g = _gen(B, T, IN, H, 7)
        x = a.inp("x", _rn(g, B, T, IN))
        w = [a.inp(n, t) for n, t in zip(("w_ih", "w_hh", "b_ih", "b_hh"), _gru_weights(g, IN, H))]
        y = a.out("y", B * T * 2 * H)
        y_last = a.out("y_last", B * 2 * H)
        ws = a.ws("ws_fwd", _ws_floats("srk_gru_top_last_workspace_floats", B, T, IN, H, 0))
        mode = _flag()
        a.call("srk_gru_top_last_fwd", x, None, B, T, IN, H, *w, y, y_last, ws, ctypes.byref(mode))
        modes.append(mode.value)
        o.add("y_last", y_last.t)
        o.add("y", y.t, written=mode.value < 2)   # modes 2, 3 leave the reverse half below the last step unwritten
        dy = a.inp("dy_last", _rn(g, B, 2 * H))
        dx = a.out("dx", B * T * IN)
        grads = _gru_grads(a, g, IN, H, accumulate)
        ws2 = a.ws("ws_bwd", _ws_floats("srk_gru_top_last_workspace_floats", B, T, IN, H, 1))
        a.call("srk_gru_top_last_bwd", x, None, B, T, IN, H, w[0], w[1], y, ws, dy, mode.value, dx, *grads, accumulate,
               ws2)
        for n, b in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), [dx] + grads):
            o.add(n, b.t)

    with precision("fp32", gru_top_last=top_last):
        run_case(fn)
    assert len(set(modes)) == 1
    assert _lib.spin_timeouts() == 0


# ----------------------------------------------------------------------------- conv
def _conv_operands(a, g, N, H, W, Ci, Co, KH, KW, ph, pw, sh, sw):
    Ho, Wo = (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1
    x = a.inp("x", _rn(g, N, H, W, Ci))
    w = a.inp("w", _rn(g, Co, Ci, KH, KW, scale=(Ci * KH * KW) ** -0.5))
    b = a.inp("bias", _rn(g, Co))
    return Ho, Wo, x, w, b


def _conv_bwd_outs(a, x, w, Co):
    return a.out("dx", x.n), a.out("dw", w.n), a.out("db", Co)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape,opts", [(s, {}) for s in CONV + [CONV_RING]] + [(CONV_RING, {"conv_ring": 0x87}),
                                                                                  (CONV_TILE256, {"conv_tile": 256})],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else
                         "-".join("%s=%s" % kv for kv in v.items()) or "default")
def test_conv2d(gpu, shape, prec, opts):
    N, H, W, Ci, Co, KH, KW, ph, pw, sh, sw = shape
    nws = _ws_floats("srk_conv2d_workspace_floats", Ci, Co, KH, KW)

    def fn(a, o):
        g = _gen(*shape)
        Ho, Wo, x, w, b = _conv_operands(a, g, *shape)
        y = a.out("y", N * Ho * Wo * Co)
        a.call("srk_conv2d_nhwc_fwd", x, N, H, W, Ci, w, b, Co, KH, KW, ph, pw, sh, sw, y, a.ws("ws_fwd", nws))
        dy = a.inp("dy", _rn(g, N, Ho, Wo, Co))
        dx, dw, db = _conv_bwd_outs(a, x, w, Co)
        a.call("srk_conv2d_nhwc_bwd", x, N, H, W, Ci, w, Co, KH, KW, ph, pw, sh, sw, dy, dx, dw, db,
               a.ws("ws_bwd", nws))
        for n, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
            o.add(n, t.t)
        dw2 = a.out("dw (dx, db null)", w.n)      # the nullable outputs null
        a.call("srk_conv2d_nhwc_bwd", x, N, H, W, Ci, w, Co, KH, KW, ph, pw, sh, sw, dy, None, dw2, None,
               a.ws("ws_bwd2", nws))
        o.add("dw (dx, db null)", dw2.t)

    with precision(prec, **opts):
        run_case(fn)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("ring", [None, 0x87])
def test_conv2d_pool(gpu, prec, ring):
    N, H, W, Ci, Co, KH, KW, ph, pw, sh, sw = CONV_RING
    nws = _ws_floats("srk_conv2d_workspace_floats", Ci, Co, KH, KW)

    def fn(a, o):
        g = _gen(*CONV_RING, 4)
        Ho, Wo, x, w, b = _conv_operands(a, g, *CONV_RING)
        npool = N * Ho * (Wo // 4) * Co
        y, arg = a.out("y", npool), a.out("argmax", npool, U8)
        x16 = a.out("x16", x.n, DT16.get(prec, torch.bfloat16))
        written = _flag()
        a.call("srk_conv2d_nhwc_fwd_pool", x, N, H, W, Ci, w, b, Co, KH, KW, ph, pw, 4, y, arg, a.ws("ws_fwd", nws), x16,
               ctypes.byref(written))
        assert written.value == (0 if prec == "fp32" else 1)
        dy = a.inp("dy_pooled", _rn(g, npool))
        dx, dw, db = _conv_bwd_outs(a, x, w, Co)
        a.call("srk_conv2d_nhwc_bwd_pool", x, N, H, W, Ci, w, Co, KH, KW, ph, pw, 4, dy, arg, dx, dw, db,
               a.ws("ws_bwd", nws), x16 if written.value else None)
        o.add("x16", x16.t, written=bool(written.value))
        for n, t in (("y", y), ("argmax", arg), ("dx", dx), ("dw", dw), ("db", db)):
            o.add(n, t.t)
        if written.value:   # x16_written = 2 on entry: the forward reads the ready copy and leaves it alone
            y2, arg2, ready = a.out("y (ready x16)", npool), a.out("argmax (ready x16)", npool, U8), ctypes.c_int(2)
            x16r = a.inp("x16 (ready)", x16.t)
            a.call("srk_conv2d_nhwc_fwd_pool", x, N, H, W, Ci, w, b, Co, KH, KW, ph, pw, 4, y2, arg2,
                   a.ws("ws_fwd2", nws), x16r, ctypes.byref(ready))
            assert same_bits(y2.t, y.t) and same_bits(arg2.t, arg.t), "the ready 16-bit copy gives other bits"
            o.add("y (ready x16)", y2.t)

    with precision(prec, **({} if ring is None else {"conv_ring": ring})):
        run_case(fn)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_conv2d_16bit_copies(gpu, prec):
    """fwd16 keeps x's 16-bit copy; bwd16, bwd16_dy16 and bwd16_acc read it (and dY's ready copy)."""
    N, H, W, Ci, Co, KH, KW, ph, pw, sh, sw = CONV_16
    nws = _ws_floats("srk_conv2d_workspace_floats", Ci, Co, KH, KW)
    geom = (Co, KH, KW, ph, pw, sh, sw)

    def fn(a, o):
        g = _gen(*CONV_16, 16)
        Ho, Wo, x, w, b = _conv_operands(a, g, *CONV_16)
        y = a.out("y", N * Ho * Wo * Co)
        x16 = a.out("x16", x.n, DT16[prec])
        written = _flag()
        a.call("srk_conv2d_nhwc_fwd16", x, N, H, W, Ci, w, b, *geom, y, a.ws("ws_fwd", nws), x16, ctypes.byref(written))
        assert written.value == 1
        o.add("y", y.t)
        o.add("x16", x16.t)
        y2, ready, x16r = a.out("y (ready x16)", y.n), ctypes.c_int(2), a.inp("x16 (ready)", x16.t)
        a.call("srk_conv2d_nhwc_fwd16", x, N, H, W, Ci, w, b, *geom, y2, a.ws("ws_fwd2", nws), x16r, ctypes.byref(ready))
        assert same_bits(y2.t, y.t), "the ready 16-bit copy gives other bits"
        o.add("y (ready x16)", y2.t)
        dyv = _rn(g, N, Ho, Wo, Co)
        dy, dy16 = a.inp("dy", dyv), a.inp("dy16", dyv.to(DT16[prec]))
        dx, dw, db = _conv_bwd_outs(a, x, w, Co)
        a.call("srk_conv2d_nhwc_bwd16", x, N, H, W, Ci, w, *geom, dy, dx, dw, db, a.ws("ws_bwd", nws), x16)
        for n, t in (("dx", dx), ("dw", dw), ("db", db)):
            o.add("bwd16." + n, t.t)
        dx, dw, db = _conv_bwd_outs(a, x, w, Co)
        a.call("srk_conv2d_nhwc_bwd16_dy16", x, N, H, W, Ci, w, *geom, dy, dy16, dx, dw, db, a.ws("ws_bwd2", nws), x16)
        for n, t in (("dx", dx), ("dw", dw), ("db", db)):
            o.add("dy16." + n, t.t)
        dx, db = a.out("dx", x.n), a.out("db", Co)
        dw = a.out("dw", w.n, init=_rn(g, w.n))
        a.call("srk_conv2d_nhwc_bwd16_acc", x, N, H, W, Ci, w, *geom, dy, dy16, dx, dw, db, a.ws("ws_bwd3", nws), x16, 1)
        for n, t in (("dx", dx), ("dw", dw), ("db", db)):
            o.add("acc." + n, t.t)

    with precision(prec):
        run_case(fn)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv1d_dilated(gpu, prec):
    N, L, Ci, Co, K, pad, dil = CONV1D_DIL
    Lo = L + 2 * pad - dil * (K - 1)
    nws = _ws_floats("srk_conv2d_workspace_floats", Ci, Co, 1, K)

    def fn(a, o):
        g = _gen(*CONV1D_DIL)
        x = a.inp("x", _rn(g, N, L, Ci))
        w = a.inp("w", _rn(g, Co, Ci, K, scale=(Ci * K) ** -0.5))
        b = a.inp("bias", _rn(g, Co))
        y = a.out("y", N * Lo * Co)
        x16 = a.out("x16", x.n, DT16.get(prec, torch.bfloat16))
        written = _flag()
        a.call("srk_conv1d_nlc_dil_fwd", x, N, L, Ci, w, b, Co, K, pad, dil, y, a.ws("ws_fwd", nws), x16,
               ctypes.byref(written))
        o.add("y", y.t)
        o.add("x16", x16.t, written=bool(written.value))
        dy = a.inp("dy", _rn(g, N, Lo, Co))
        dx, dw, db = _conv_bwd_outs(a, x, w, Co)
        a.call("srk_conv1d_nlc_dil_bwd", x, N, L, Ci, w, Co, K, pad, dil, dy, None, dx, dw, db, a.ws("ws_bwd", nws),
               x16 if written.value else None, 0)
        for n, t in (("dx", dx), ("dw", dw), ("db", db)):
            o.add(n, t.t)

    with precision(prec):
        run_case(fn)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N,H,W,KH,KW,pool", CONV1_POOL)
def test_conv1_pool(gpu, prec, N, H, W, KH, KW, pool):
    Co, ph, pw, Wp = 64, KH // 2, KW // 2, W // pool

    def fn(a, o):
        g = _gen(N, H, W, KH, KW, pool)
        x = a.inp("x", _rn(g, N, H, W, scale=30.0))
        w = a.inp("w", _rn(g, Co, 1, KH, KW, scale=0.2))
        b = a.inp("bias", _rn(g, Co))
        n = N * H * Wp * Co
        y, arg = a.out("y", n), a.out("argmax", n, U8)
        a.call("srk_conv1_pool_fwd", x, N, H, W, w, b, Co, KH, KW, ph, pw, pool, y, arg)
        o.add("y", y.t)
        o.add("argmax", arg.t)
        y2, arg2 = a.out("y (fwd16)", n), a.out("argmax (fwd16)", n, U8)
        y16 = a.out("y16", n, DT16.get(prec, torch.bfloat16))
        written = _flag()
        a.call("srk_conv1_pool_fwd16", x, N, H, W, w, b, Co, KH, KW, ph, pw, pool, y2, arg2, y16, ctypes.byref(written))
        assert written.value == (0 if prec == "fp32" else 1)
        o.add("fwd16.y", y2.t)
        o.add("fwd16.argmax", arg2.t)
        o.add("fwd16.y16", y16.t, written=bool(written.value))
        y3, arg3, y16c, only = a.out("y (copy only)", n), a.out("argmax (copy only)", n, U8), \
            a.out("y16 (copy only)", n, DT16.get(prec, torch.bfloat16)), ctypes.c_int(3)
        a.call("srk_conv1_pool_fwd16", x, N, H, W, w, b, Co, KH, KW, ph, pw, pool, y3, arg3, y16c, ctypes.byref(only))
        if only.value:      # the copy was written: y is left alone
            assert same_bits(y16c.t, y16.t) and _never_written(y3.t) == n
        o.add("copy-only.y", y3.t, written=not only.value)
        o.add("copy-only.argmax", arg3.t)
        o.add("copy-only.y16", y16c.t, written=bool(only.value))
        dy = a.inp("dy", _rn(g, n))
        dw, db = a.out("dw", Co * KH * KW), a.out("db", Co)
        a.call("srk_conv1_pool_wgrad", x, N, H, W, Co, KH, KW, ph, pw, pool, dy, arg, dw, db,
               a.ws("ws", _ws_floats("srk_conv1_pool_workspace_floats", Co, KH, KW)))
        o.add("dw", dw.t)
        o.add("db", db.t)
        if W % pool == 0:   # the data gradient accepts only W % pool == 0
            dx = a.out("dx", N * H * W)
            a.call("srk_conv1_pool_dgrad", w, N, H, W, Co, KH, KW, ph, pw, pool, dy, arg, dx)
            o.add("dx", dx.t)

    with precision(prec):
        run_case(fn)


@pytest.mark.parametrize("N,H,W,C,kh,kw", MAXPOOL)
def test_maxpool(gpu, N, H, W, C, kh, kw):
    def fn(a, o):
        g = _gen(N, H, W, C)
        x = a.inp("x", _rn(g, N, H, W, C))
        n = N * (H // kh) * (W // kw) * C
        y = a.out("y", n)
        a.call("srk_maxpool_nhwc_fwd", x, N, H, W, C, kh, kw, y)
        dy = a.inp("dy", _rn(g, n))
        dx = a.out("dx", x.n)
        a.call("srk_maxpool_nhwc_bwd", x, dy, N, H, W, C, kh, kw, dx)
        o.add("y", y.t)
        o.add("dx", dx.t)

    run_case(fn)


# ----------------------------------------------------------------------------- batch norm
@pytest.mark.parametrize("nulls", [False, True], ids=["all-outputs", "nullable-outputs-null"])
@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("training", [0, 1])
@pytest.mark.parametrize("M,C", BN)
def test_batchnorm(gpu, M, C, training, relu, residual, nulls):
    eps, mom, dt = 1e-5, 0.1, torch.bfloat16

    def fn(a, o):
        g = _gen(M, C)
        xv = _rn(g, M, C, scale=2.0) + 0.5
        x, dy = a.inp("x", xv), a.inp("dy", _rn(g, M, C))
        gamma, beta = a.inp("gamma", _rn(g, C) * 0.5 + 1.0), a.inp("beta", _rn(g, C))
        res = a.inp("residual", _rn(g, M, C)) if residual else None
        rm0, rv0 = _rn(g, C, scale=0.1) + 0.5, torch.rand(C, generator=g).cuda() + 3.5

        def opt(name, n, dtype=F32, init=None):
            return None if nulls else a.out(name, n, dtype, init=init)

        def fwd(tag, entry, extra):
            rm, rv = a.out(tag + "running_mean", C, init=rm0), a.out(tag + "running_var", C, init=rv0)
            y, sm, si = a.out(tag + "y", M * C), a.out(tag + "save_mean", C), a.out(tag + "save_invstd", C)
            a.call(entry, x, M, C, gamma, beta, eps, mom, training, rm, rv, res, relu, y, *extra, sm, si)
            for n, b in (("running_mean", rm), ("running_var", rv), ("y", y), ("save_mean", sm), ("save_invstd", si)):
                o.add(tag + n, b.t)
            return y, sm, si

        def bwd(tag, entry, y, sm, si, pre=(), mid=(), post=()):
            dx, dres = opt(tag + "dx", M * C), opt(tag + "dresidual", M * C)
            dg, db = a.out(tag + "dgamma", C), a.out(tag + "dbeta", C)
            a.call(entry, x, y, *pre, dy, M, C, gamma, sm, si, training, relu, dx, *mid, dg, db, dres, *post)
            for n, b in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("dresidual", dres)):
                if b is not None:
                    o.add(tag + n, b.t)

        y, sm, si = fwd("", "srk_batchnorm_fwd", ())
        bwd("", "srk_batchnorm_bwd", y, sm, si)
        # the 16-bit copies, the accumulating form and the ReLU bit mask
        y16, wr = opt("y16", M * C, dt), _flag()
        y, sm, si = fwd("f16.", "srk_batchnorm_fwd16", (y16, ctypes.byref(wr)))
        assert wr.value == (0 if nulls else 1)
        dx16, wr = opt("dx16", M * C, dt), _flag()
        bwd("b16.", "srk_batchnorm_bwd16", y, sm, si, mid=(dx16, ctypes.byref(wr)))
        assert wr.value == (0 if nulls else 1)
        dx16b, ga, ba = opt("acc.dx16", M * C, dt), opt("dgamma_acc", C, init=_rn(g, C)), opt("dbeta_acc", C, init=_rn(g, C))
        bwd("acc.", "srk_batchnorm_bwd16_acc", y, sm, si, mid=(dx16b, ctypes.byref(wr)), post=(ga, ba))
        y16m, mask, wr = opt("mask.y16", M * C, dt), opt("relu_mask", M * C // 4, U8), _flag()
        y, sm, si = fwd("mask.", "srk_batchnorm_fwd16_mask", (y16m, ctypes.byref(wr), mask))
        dx16m, gm, bm = opt("mask.dx16", M * C, dt), opt("mask.dgamma_acc", C, init=_rn(g, C)), opt("mask.dbeta_acc", C, init=_rn(g, C))
        bwd("bmask.", "srk_batchnorm_bwd16_mask", y, sm, si, pre=(mask,), mid=(dx16m, ctypes.byref(wr)), post=(gm, bm))
        for n, b in (("y16", y16), ("dx16", dx16), ("acc.dx16", dx16b), ("dgamma_acc", ga), ("dbeta_acc", ba),
                     ("mask.y16", y16m), ("mask.dx16", dx16m), ("mask.dgamma_acc", gm), ("mask.dbeta_acc", bm)):
            if b is not None:
                o.add(n, b.t)
        if mask is not None:
            o.add("relu_mask", mask.t, written=bool(relu))

    with precision("bf16"):
        run_case(fn)


@pytest.mark.parametrize("nulls", [False, True], ids=["all-outputs", "nullable-outputs-null"])
@pytest.mark.parametrize("residual", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("M,C", BN)
def test_sync_batchnorm_pieces(gpu, M, C, relu, residual, nulls):
    eps, mom, world = 1e-5, 0.1, 2

    def fn(a, o):
        g = _gen(M, C, 5)
        x, dy = a.inp("x", _rn(g, M, C, scale=2.0) + 0.5), a.inp("dy", _rn(g, M, C))
        gamma, beta = a.inp("gamma", _rn(g, C) * 0.5 + 1.0), a.inp("beta", _rn(g, C))
        res = a.inp("residual", _rn(g, M, C)) if residual else None
        stats = a.out("stats", 3 * C)
        a.call("srk_batchnorm_stats", x, M, C, stats)
        o.add("stats", stats.t)
        both = a.inp("stats_all", torch.cat([stats.t, stats.t]))     # two ranks with the same rows
        rm = None if nulls else a.out("running_mean", C, init=_rn(g, C, scale=0.1))
        rv = None if nulls else a.out("running_var", C, init=torch.rand(C, generator=g).cuda() + 0.5)
        sm, si = a.out("save_mean", C), a.out("save_invstd", C)
        total = a.out("total_count", 1)
        a.call("srk_batchnorm_combine", both, world, C, eps, mom, rm, rv, sm, si, total)
        y = a.out("y", M * C)
        a.call("srk_batchnorm_apply", x, M, C, sm, si, gamma, beta, res, relu, y)
        sums = a.out("sums", 2 * C)
        a.call("srk_batchnorm_bwd_reduce", x, y, dy, M, C, sm, si, relu, sums)
        dx = a.out("dx", M * C)
        dres = None if nulls else a.out("dresidual", M * C)
        a.call("srk_batchnorm_bwd_dx", x, y, dy, M, C, total, gamma, sm, si, sums, relu, dx, dres)
        for n, b in (("running_mean", rm), ("running_var", rv), ("save_mean", sm), ("save_invstd", si),
                     ("total_count", total), ("y", y), ("sums", sums), ("dx", dx), ("dresidual", dres)):
            if b is not None:
                o.add(n, b.t)

    run_case(fn)


# ----------------------------------------------------------------------------- step ops
@pytest.mark.parametrize("B,C,lead", CE)
@pytest.mark.parametrize("with_grad", [True, False])
def test_cross_entropy(gpu, B, C, lead, with_grad):
    def fn(a, o):
        g = _gen(B, C)
        logits = a.inp("logits", _rn(g, B, C, scale=3.0), lead=lead)
        labels = a.inp("labels", torch.randint(0, C, (B,), generator=g).cuda())
        loss = a.out("loss", 1, lead=lead)
        dl = a.out("dlogits", B * C, lead=lead) if with_grad else None
        a.call("srk_cross_entropy", logits, labels, B, C, loss, dl, a.ws("ws", B + 1))
        o.add("loss", loss.t)
        if dl is not None:
            o.add("dlogits", dl.t)

    run_case(fn)


def _adam_state(lr):
    st = torch.zeros(8, dtype=F32)
    st[4] = lr
    return st.view(I64).cuda()


@pytest.mark.parametrize("n", ADAM_N)
def test_adam(gpu, n):
    def fn(a, o):
        g = _gen(n)
        p0, m0, v0 = _rn(g, n), _rn(g, n, scale=0.01), _rn(g, n, scale=0.01).abs()
        grad = a.inp("grad", _rn(g, n))
        for tag, entry in (("", "srk_adam_step"), ("state.", "srk_adam_step_state"), ("scaled.", "srk_adam_step_scaled")):
            p, m, v = a.out(tag + "param", n, init=p0), a.out(tag + "exp_avg", n, init=m0), a.out(tag + "exp_avg_sq", n, init=v0)
            bufs = [("param", p), ("exp_avg", m), ("exp_avg_sq", v)]
            if entry == "srk_adam_step":
                a.call(entry, p, grad, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5)
            else:
                st = a.out(tag + "state", 4, I64, init=_adam_state(1e-3))
                bufs.append(("state", st))
                if entry == "srk_adam_step_state":
                    a.call(entry, p, grad, m, v, n, 0.9, 0.999, 1e-8, st, 0.5)
                else:
                    sc = a.out("scaler", 8, I32)
                    a.call("srk_grad_scaler_init", sc, 1024.0, 2.0, 0.5, 2)
                    a.call(entry, p, grad, m, v, n, 0.9, 0.999, 1e-8, st, 0.5, sc)
                    bufs.append(("scaler", sc))
            for name, b in bufs:
                o.add(tag + name, b.t)

    run_case(fn)


@pytest.mark.parametrize("n,lead", DROPOUT)
def test_dropout_and_uniform(gpu, n, lead):
    def fn(a, o):
        g = _gen(n, lead)
        x = a.inp("x", _rn(g, n), lead=lead)
        y, keep = a.out("y", n, lead=lead), a.out("keep", n, U8, lead=lead)
        a.call("srk_dropout_fwd", x, n, 0.3, ctypes.c_uint64(0x1234567887654321), y, keep)
        st = a.out("state", 2, I64, init=torch.tensor([0x5EED5EED, 3], dtype=I64))
        y2, keep2 = a.out("y (state)", n, lead=lead), a.out("keep (state)", n, U8, lead=lead)
        a.call("srk_dropout_fwd_state", x, n, 0.3, st, y2, keep2)
        y3 = a.out("y (apply)", n, lead=lead)
        a.call("srk_dropout_apply", x, keep, n, 1.0 / 0.7, y3)
        st2 = a.out("uniform state", 2, I64, init=torch.tensor([0x5EED, 1], dtype=I64))
        u = a.out("u", n, F64)
        a.call("srk_uniform_f64_state", st2, 0.9, 1.1, n, u)
        for name, b in (("y", y), ("keep", keep), ("state", st), ("state.y", y2), ("state.keep", keep2), ("apply.y", y3),
                        ("uniform.state", st2), ("u", u)):
            o.add(name, b.t)

    got = run_case(fn)
    assert int(got["state"][1]) == 4 and int(got["uniform.state"][1]) == 2
    assert bool(((got["u"] >= 0.9) & (got["u"] < 1.1)).all())


@pytest.mark.parametrize("K,B,C,lead", ENSEMBLE)
@pytest.mark.parametrize("nulls", [False, True])
def test_softmax_ensemble(gpu, K, B, C, lead, nulls):
    def fn(a, o):
        logits = a.inp("logits", _rn(_gen(K, B, C), K, B, C, scale=3.0), lead=lead)
        cat = None if nulls else a.out("probs_cat", B * K * C, lead=lead)
        mean = a.out("mean", B * C, lead=lead)
        pred = None if nulls else a.out("pred", B, I64)
        a.call("srk_softmax_ensemble", logits, K, B, C, cat, mean, pred)
        for name, b in (("probs_cat", cat), ("mean", mean), ("pred", pred)):
            if b is not None:
                o.add(name, b.t)

    run_case(fn)


# ----------------------------------------------------------------------------- features and augmentation
def _pcm(g, n):
    return torch.randint(-20000, 20000, (n, 16000), generator=g, dtype=I16)


def test_features(gpu):
    """n = 3 clips through every srk_fbank / mfcc / spec entry: both PCM dtypes, both layouts, VTLP."""
    n = 3

    def fn(a, o):
        g = _gen(n, 16000)
        p16 = _pcm(g, n)
        pcm = {"": a.inp("pcm", p16.float().cuda()), "_i16": a.inp("pcm_i16", p16.cuda())}
        alpha = a.inp("alpha", torch.tensor([0.9, 1.0, 1.1], dtype=F64).cuda())
        for sfx, p in pcm.items():
            out = a.out("fbank" + sfx, n * 98 * 120)
            a.call("srk_fbank_fwd" + sfx, p, n, out)
            o.add("fbank" + sfx, out.t)
            out = a.out("fbank_vtlp" + sfx, n * 98 * 120)
            a.call("srk_fbank_vtlp_fwd" + sfx, p, n, alpha, out)
            o.add("fbank_vtlp" + sfx, out.t)
            for layout in (0, 1):
                out = a.out("mfcc%s layout %d" % (sfx, layout), n * 39 * 51)
                a.call("srk_mfcc_fwd" + sfx, p, n, out, layout)
                o.add("mfcc%s.%d" % (sfx, layout), out.t)
                out = a.out("spec%s transposed %d" % (sfx, layout), n * 321 * 49)
                a.call("srk_spec_fwd" + sfx, p, n, out, layout)
                o.add("spec%s.%d" % (sfx, layout), out.t)

    run_case(fn)


def test_noise_mix_window_ends_on_the_banks_last_sample(gpu):
    n, n_files, bank_len = 3, 2, 16000 + 124

    def fn(a, o):
        g = _gen(n, bank_len)
        pcm = a.inp("pcm", _pcm(g, n).cuda())
        bank = a.inp("bank", torch.randint(-3000, 3000, (n_files, bank_len), generator=g, dtype=I16).cuda())
        fi = a.inp("file_idx", torch.tensor([0, 1, 1], dtype=I64).cuda())
        off = a.inp("offset", torch.tensor([0, 57, bank_len - 16000], dtype=I64).cuda())
        gain = a.inp("gain", torch.tensor([0.1, 0.25, 0.5], dtype=F64).cuda())
        out = a.out("out", n * 16000)
        a.call("srk_noise_mix", pcm, bank, n_files, bank_len, fi, off, gain, n, out)
        o.add("mixed", out.t)
        for tr in (0, 1):
            s = a.out("spec %d" % tr, n * 321 * 49)
            a.call("srk_spec_noise_fwd", pcm, bank, n_files, bank_len, fi, off, gain, n, s, tr)
            o.add("spec.%d" % tr, s.t)

    run_case(fn)


def test_augment_one_clip_per_op(gpu):
    ops = [0, 1, 1, 2, 2, 3, 4, 5, 5, 6]
    n, bank_len = len(ops), 16000 + 333
    last = bank_len - 16000
    iparam = [0, 14400, 17600, 1234, -4321, 0, 0, 0, 0, 1]
    pos = [0, 0, 0, 0, 0, last, last, last, -1, 0]
    dparam = [0.0, 0.0, 0.0, 0.0, 0.0, 0.3, 10.0, 0.5, 0.5, 0.0]

    def fn(a, o):
        g = _gen(n, bank_len)
        pcm = a.inp("pcm", _pcm(g, n).cuda())
        bank = a.inp("bank", torch.randint(-3000, 3000, (bank_len,), generator=g, dtype=I16).cuda())
        op = a.inp("op", torch.tensor(ops, dtype=I32).cuda())
        ip = a.inp("iparam", torch.tensor(iparam, dtype=I64).cuda())
        ps = a.inp("noise_pos", torch.tensor(pos, dtype=I64).cuda())
        dp = a.inp("dparam", torch.tensor(dparam, dtype=F64).cuda())
        out = a.out("out", n * 16000)
        a.call("srk_augment", pcm, n, bank, bank_len, op, ip, ps, dp, ctypes.c_uint64(99), out)
        o.add("augmented", out.t)

    run_case(fn)


def test_pitch_shift_clip_subset(gpu):
    n, idx, lvl = 3, [2, 0], [0, 3]
    nbytes = _ws_floats("srk_pitch_workspace_bytes", len(idx))

    def fn(a, o):
        p16 = _pcm(_gen(n, 12), n)
        pcm = a.inp("pcm", p16.cuda())
        ci, li = a.inp("clip_idx", torch.tensor(idx, dtype=I32).cuda()), a.inp("level_idx", torch.tensor(lvl, dtype=I32).cuda())
        out = a.out("out", n * 16000, init=p16.float())
        a.call("srk_pitch_shift", pcm, n, ci, li, len(idx), out, a.ws("ws", nbytes, U8), nbytes)
        o.add("shifted", out.t)

    got = run_case(fn)
    assert not torch.equal(got["shifted"].view(n, 16000)[0], got["shifted"].view(n, 16000)[1])


# ----------------------------------------------------------------------------- newer ops
@pytest.mark.parametrize("B,T,D,lead", ATTN)
@pytest.mark.parametrize("regs", [1, 0])
def test_attn_pool(gpu, B, T, D, lead, regs):
    scale = D ** -0.5

    def fn(a, o):
        g = _gen(B, T, D)
        y, q = a.inp("y", _rn(g, B, T, D), lead=lead), a.inp("q", _rn(g, B, D), lead=lead)
        ctx, alpha = a.out("ctx", B * D, lead=lead), a.out("alpha", B * T, lead=lead)
        a.call("srk_attn_pool_fwd", y, q, B, T, D, scale, ctx, alpha)
        dctx = a.inp("dctx", _rn(g, B, D), lead=lead)
        dy, dq = a.out("dy", B * T * D, lead=lead), a.out("dq", B * D, lead=lead)
        a.call("srk_attn_pool_bwd", y, q, alpha, dctx, B, T, D, scale, dy, dq)
        for name, b in (("ctx", ctx), ("alpha", alpha), ("dy", dy), ("dq", dq)):
            o.add(name, b.t)

    with _lib.options(attn_pool_regs=regs):
        run_case(fn)


@pytest.mark.parametrize("B,T,C", PCEN)
@pytest.mark.parametrize("null", [None, "m_out", "dx"])
def test_pcen(gpu, B, T, C, null):
    ls, eps = math.log(10.0) / 20.0, 1e-6
    nws = _ws_floats("srk_pcen_workspace_floats", B, T, C)

    def fn(a, o):
        g = _gen(B, T, C)
        x = a.inp("x", _rn(g, B, T, C, scale=10.0))
        p0 = torch.tensor([math.log(0.98), math.log(2.0), math.log(0.5), math.log(0.04 / 0.96)])[:, None]
        p = a.inp("p", (p0 + 0.05 * torch.randn(4, C, generator=g)).cuda())
        y, m = a.out("y", x.n), a.out("m", x.n)
        a.call("srk_pcen_fwd", x, p, B, T, C, ls, eps, y, m)
        if null == "m_out":
            y2 = a.out("y (no m)", x.n)
            a.call("srk_pcen_fwd", x, p, B, T, C, ls, eps, y2, None)
            o.add("y (no m)", y2.t)
        dy = a.inp("dy", _rn(g, B, T, C))
        dx = None if null == "dx" else a.out("dx", x.n)
        dp = a.out("dp", 4 * C)
        a.call("srk_pcen_bwd", x, p, m, dy, B, T, C, ls, eps, dx, dp, a.ws("ws", nws))
        for name, b in (("y", y), ("m", m), ("dx", dx), ("dp", dp)):
            if b is not None:
                o.add(name, b.t)

    run_case(fn)


@pytest.mark.parametrize("N,H,W,C,KH,KW,ph,pw,sh,sw,lead", DWCONV)
@pytest.mark.parametrize("variant", ["plain", "db-null", "dw-accumulate", "dx-null"])
def test_dwconv(gpu, N, H, W, C, KH, KW, ph, pw, sh, sw, lead, variant):
    Ho, Wo = (H + 2 * ph - KH) // sh + 1, (W + 2 * pw - KW) // sw + 1
    nws = _ws_floats("srk_dwconv2d_workspace_floats", N, H, W, C, KH, KW, ph, pw, sh, sw)
    assert nws > 0

    def fn(a, o):
        g = _gen(N, H, W, C, sh, sw)
        x = a.inp("x", _rn(g, N, H, W, C), lead=lead)
        w = a.inp("w", _rn(g, C, 1, KH, KW, scale=0.3), lead=lead)
        b = a.inp("bias", _rn(g, C), lead=lead)
        y = a.out("y", N * Ho * Wo * C, lead=lead)
        a.call("srk_dwconv2d_nhwc_fwd", x, N, H, W, C, w, b, KH, KW, ph, pw, sh, sw, y)
        dy = a.inp("dy", _rn(g, N, Ho, Wo, C), lead=lead)
        dx = None if variant == "dx-null" else a.out("dx", x.n, lead=lead)
        acc = int(variant == "dw-accumulate")
        dw = a.out("dw", w.n, init=_rn(g, w.n) if acc else None, lead=lead)
        db = None if variant == "db-null" else a.out("db", C, lead=lead)
        a.call("srk_dwconv2d_nhwc_bwd", x, N, H, W, C, w, KH, KW, ph, pw, sh, sw, dy, dx, dw, db, a.ws("ws", nws), acc)
        for name, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
            if t is not None:
                o.add(name, t.t)

    run_case(fn)


@pytest.mark.parametrize("N,HW,C", AVGPOOL)
def test_avgpool(gpu, N, HW, C):
    def fn(a, o):
        g = _gen(N, HW, C)
        x = a.inp("x", _rn(g, N, HW, C))
        y = a.out("y", N * C)
        a.call("srk_avgpool_nhwc_fwd", x, N, HW, C, y)
        dy = a.inp("dy", _rn(g, N, C))
        dx = a.out("dx", x.n)
        a.call("srk_avgpool_nhwc_bwd", dy, N, HW, C, dx)
        o.add("y", y.t)
        o.add("dx", dx.t)

    run_case(fn)


@pytest.mark.parametrize("T,F", SPECAUG)
@pytest.mark.parametrize("time_major", [1, 0])
@pytest.mark.parametrize("in_place", [False, True])
def test_specaug(gpu, T, F, time_major, in_place):
    B, W, NF, f_max, NT, t_max = 3, 5, 2, 8, 2, 10
    P = 2 + 2 * NF + 2 * NT

    def fn(a, o):
        g = _gen(T, F, time_major)
        xv = _rn(g, B, T * F)
        st = a.out("state", 2, I64, init=torch.tensor([0xABCDEF, 2], dtype=I64))
        params = a.out("params", B * P, I32)
        a.call("srk_specaug_draw", st, B, T, F, W, NF, f_max, NT, t_max, params)
        o.add("state", st.t)
        o.add("params", params.t)
        for fill_mode in (0, 1):
            if in_place:
                x = y = a.out("x = y (fill %d)" % fill_mode, B * T * F, init=xv)
            else:
                x, y = a.inp("x", xv), a.out("y (fill %d)" % fill_mode, B * T * F)
            a.call("srk_specaug_apply", x, B, T, F, time_major, params, NF, NT, fill_mode, -1.5, y)
            o.add("y.%d" % fill_mode, y.t)

    got = run_case(fn)
    assert int(got["state"][1]) == 3


# ----------------------------------------------------------------------------- diagnostics entry points
def test_diag_entry_points(gpu):
    def fn(a, o):
        rows = 16
        dx = a.out("dx", rows * 40 * 64, init=torch.full((rows * 40 * 64,), -1.0))
        a.call("srk_diag_acc_store", dx, rows, 0)
        o.add("dx", dx.t)
        for cols in (64, 128):
            m = a.inp("m", torch.randint(-32768, 32767, (32, cols), generator=_gen(cols), dtype=I16).cuda())
            out = a.out("out", (cols // 32) * 2 * 64 * 4, I32)
            a.call("srk_diag_tr16_read", m, cols, out)
            o.add("tr16.%d" % cols, out.t)

    run_case(fn)
