"""BiGRU.forward_last (srk_gru_top_last_fwd / _bwd): row T-1 of the top layer for the models that read nothing else.

The reference is torch.nn.GRU on the CPU in float64 with the same weights (out[:, -1, :], then autograd).  y_last is
held to tolerances.LOGITS_REL and every parameter gradient and dx to 2e-3 (test_models_gpu.py's bound), both with
rel_err; the top layer's weight_hh_l{top}_reverse, whose true gradient is exactly zero (the one live reverse step
has h_prev = 0), must come out as exact zeros.  Shapes: H = 512 (the persistent kernels' size), the smallest (B, T)
that reach every branch: T = 1 (K = B T - 1 = 0 in dW_hh), a partial 64-row group (65), two recurrence chunks
(300), the fused layer-0 / top-layer projection (in = 39 / 40), a top layer behind a GEMM projection (in = 1024).
Off the fp32 persistent path the entry points run the full layer, so there the results equal
last_step(forward(x)[0]) bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import nn as snn
from speechrecognitionproject_amd.graphs import GraphedStep
from speechrecognitionproject_amd.optim import Adam, FlatParams
from tolerances import LOGITS_REL, rel_err

GRAD_REL = 2e-3
# option gru_top_last on the fp32 persistent path: 1 the pruned backward GEMMs, 2 also the reverse direction as one
# cell (the pruned dW_ih pair, the forward-half dx plus the B-row add), 3 that cell with the full dW_ih / dx GEMMs
# (the default).  Every shape, accumulate and graph test runs in each of them.
MODES = [1, 2, 3]
DEFAULT_MODE = 3


def _mode(mode):
    return _lib.options(gru_top_last=mode)


def _inputs(layers, IN, H, B, T, seed):
    """(float64 torch.nn.GRU with seeded weights, its state_dict in float32, x, g)."""
    gen = torch.Generator().manual_seed(seed)
    ref = torch.nn.GRU(IN, H, layers, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.empty(p.shape, dtype=torch.float64).uniform_(-H ** -0.5, H ** -0.5, generator=gen))
    x = torch.randn(B, T, IN, generator=gen)
    g = torch.randn(B, 2 * H, generator=gen)
    return ref, {k: v.detach().float() for k, v in ref.state_dict().items()}, x, g


@functools.lru_cache(maxsize=None)
def _reference(layers, IN, H, B, T, seed):
    """(state_dict, x, g, y_last, {name: grad}, dx) of torch.nn.GRU in float64 on the CPU; the loss is
    sum(y_last * g) with a fixed random g.  Computed once per case and shared by the modes."""
    ref, sd, x, g = _inputs(layers, IN, H, B, T, seed)
    xd = x.double().requires_grad_(True)
    out, _ = ref(xd)
    y_last = out[:, -1, :]
    (y_last * g.double()).sum().backward()
    grads = {k: p.grad.clone() for k, p in ref.named_parameters()}
    return sd, x, g, y_last.detach(), grads, xd.grad.clone()


def _device_gru(layers, IN, H, sd):
    gru = snn.BiGRU(IN, H, num_layers=layers).cuda()
    gru.load_state_dict(sd)
    return gru


def _run(gru, x, g, x_grad, last=True):
    """(y_last, {name: grad}, dx or None) of forward_last (last) or last_step(forward(x)[0]) on the device."""
    for p in gru.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(x_grad)
    y = gru.forward_last(xg) if last else snn.last_step(gru(xg)[0])
    (y * g.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in gru.named_parameters()}
    return y.detach().clone(), grads, (xg.grad.detach().clone() if x_grad else None)


def _check_against(tag, y, grads, dx, ry, rgrads, rdx, zero_name):
    e = rel_err(y.cpu().double(), ry)
    print("%s y_last rel %.3g" % (tag, e))
    errs = {}
    for k, rg in rgrads.items():
        if k == zero_name:
            continue
        errs[k] = rel_err(grads[k].cpu().double(), rg)
        print("%s d%s rel %.3g" % (tag, k, errs[k]))
    edx = rel_err(dx.cpu().double(), rdx) if dx is not None else None
    if edx is not None:
        print("%s dx rel %.3g" % (tag, edx))
    nz = int(torch.count_nonzero(grads[zero_name]))
    print("%s d%s non-zeros %d" % (tag, zero_name, nz))
    assert e <= LOGITS_REL, (tag, e)
    for k, v in errs.items():
        assert v <= GRAD_REL, (tag, k, v)
    assert edx is None or edx <= GRAD_REL, (tag, edx)
    assert float(rgrads[zero_name].abs().max()) == 0.0   # the reference agrees that it is exactly zero
    assert nz == 0, (tag, zero_name, nz)


# the last two: a top layer whose input width is no multiple of 4 (the zero-padded x / W_ih / dW_ih / dx copies), with
# and without dx
CASES = [(2, 39, 1, 1, False), (2, 39, 1, 2, False), (2, 39, 65, 5, False), (2, 39, 300, 3, False),
         (1, 40, 8, 4, False), (1, 1024, 64, 2, True), (1, 1024, 64, 2, False), (1, 1023, 9, 3, True),
         (1, 1023, 9, 3, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layers,IN,B,T,x_grad", CASES)
def test_forward_last_matches_float64_gru(gpu, layers, IN, B, T, x_grad, mode):
    sd, x, g, ry, rgrads, rdx = _reference(layers, IN, 512, B, T, 3)
    gru = _device_gru(layers, IN, 512, sd)
    with _mode(mode):
        y, grads, dx = _run(gru, x, g, x_grad)
    assert y.shape == (B, 1024) and y.is_contiguous()
    _check_against("mode %d L%d in%d B%d T%d" % (mode, layers, IN, B, T), y, grads, dx, ry, rgrads,
                   rdx if x_grad else None, "weight_hh_l%d_reverse" % (layers - 1))
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_forward_last_modes_match_full_layer(gpu, mode):
    """Every gru_top_last mode (0 the full layer, 1 the pruned backward GEMMs, 2 also the reverse direction as one
    cell, 3 that cell with the full dW_ih / dx GEMMs; 3 is the default) against last_step(forward(x)[0]) of the same
    module and against the float64 reference: values and all gradients within the same tolerances (the GEMM shapes
    differ in modes 1 and 2, and at this small shape the K splits in mode 3, so not bitwise)."""
    sd, x, g, ry, rgrads, rdx = _reference(2, 39, 512, 65, 5, 5)
    gru = _device_gru(2, 39, 512, sd)
    fy, fgrads, fdx = _run(gru, x, g, True, last=False)
    with _mode(mode):
        y, grads, dx = _run(gru, x, g, True)
    e = rel_err(y.cpu(), fy.cpu())
    print("mode %d vs full layer: y_last rel %.3g" % (mode, e))
    assert e <= LOGITS_REL
    for k in fgrads:
        ek = rel_err(grads[k].cpu(), fgrads[k].cpu())
        print("mode %d vs full layer: d%s rel %.3g" % (mode, k, ek))
        assert ek <= GRAD_REL, (k, ek)
    edx = rel_err(dx.cpu(), fdx.cpu())
    print("mode %d vs full layer: dx rel %.3g" % (mode, edx))
    assert edx <= GRAD_REL
    _check_against("mode %d" % mode, y, grads, dx, ry, rgrads, rdx, "weight_hh_l1_reverse")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_forward_last_accumulates_in_place(gpu, mode):
    """FlatParams + Adam (the kernels add into .grad in place) against plain parameters on the same inputs, and two
    backward passes without zero_grad: twice the gradient, within 1e-6 relative (dW_hh[1] is left alone: zero)."""
    with _mode(mode):
        _accumulates_in_place()


def _accumulates_in_place():
    sd, x, g, _, _, _ = _reference(2, 39, 512, 65, 5, 7)
    plain = _device_gru(2, 39, 512, sd)
    _, pgrads, pdx = _run(plain, x, g, True)
    gru = _device_gru(2, 39, 512, sd)
    flat = FlatParams(gru.parameters())
    opt = Adam(gru.parameters(), lr=1e-4, flat=flat)
    opt.zero_grad()
    xg = x.cuda().requires_grad_(True)

    def backward_once():
        xg.grad = None
        (gru.forward_last(xg) * g.cuda()).sum().backward()
        torch.cuda.synchronize()

    backward_once()
    assert all(flat.owns_grad(p) for p in gru.parameters())   # still the flat buffer's views: accumulated in place
    once = flat.grad.clone()
    for k, p in gru.named_parameters():
        e = rel_err(p.grad.cpu(), pgrads[k].cpu())
        print("in place vs plain: d%s rel %.3g" % (k, e))
        assert e <= 1e-6, (k, e)
    assert rel_err(xg.grad.cpu(), pdx.cpu()) <= 1e-6
    backward_once()
    e2 = rel_err(flat.grad.cpu(), 2.0 * once.cpu())
    print("two backward passes vs twice one: rel %.3g" % e2)
    assert e2 <= 1e-6
    assert int(torch.count_nonzero(gru.weight_hh_l1_reverse.grad)) == 0


def _bitwise_vs_full(layers, IN, H, B, T):
    _, sd, x, g = _inputs(layers, IN, H, B, T, 11)
    gru = _device_gru(layers, IN, H, sd)
    fy, fgrads, fdx = _run(gru, x, g, True, last=False)
    y, grads, dx = _run(gru, x, g, True)
    assert torch.equal(y, fy)
    for k in fgrads:
        assert torch.equal(grads[k], fgrads[k]), k
    assert torch.equal(dx, fdx)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_forward_last_16bit_is_the_full_layer(gpu, precision):
    try:
        _lib.set_matmul_precision(precision)
        _bitwise_vs_full(2, 39, 512, 8, 4)
    finally:
        _lib.set_matmul_precision("fp32")


@pytest.mark.gpu
def test_forward_last_without_persistent_kernels_is_the_full_layer(gpu):
    with _lib.options(gru_persistent=0):
        _bitwise_vs_full(2, 39, 512, 8, 4)


@pytest.mark.gpu
def test_forward_last_other_hidden_size_is_the_full_layer(gpu):
    _bitwise_vs_full(2, 39, 128, 8, 4)   # H = 128: admitted by the layer, not by the persistent kernels


@pytest.mark.gpu
@pytest.mark.parametrize("IN,B,T", [(256, 65, 5), (1024, 256, 51)])
def test_forward_last_default_mode_has_the_full_layers_bits(gpu, IN, B, T):
    """Mode 3 keeps every sum in the full layer's order, so y_last, every gradient and dx equal
    last_step(forward(x)[0]) BIT FOR BIT wherever the layer's input projection runs as one unsplit GEMM: K = in < 512
    is never split, and (256, 51, 1024) is the benchmark's top layer.  This pins what the mode rests on: an element's
    sum order depends on the GEMM kernel and its K split, not on the tile shape (64 x 64 for the B-row projection,
    256 x 128 for the full one) nor on the tile grid (the forward-only dW_hh planned as the two-direction launch)."""
    with _mode(DEFAULT_MODE):
        _bitwise_vs_full(1, IN, 512, B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_forward_last_graph_replays_equal_eager_step(gpu, mode):
    """forward + backward + Adam at (8, 4) captured into a HIP graph: two replays from the same state are bitwise
    equal to each other and to the eager step from that state."""
    with _mode(mode):
        _graph_replays_equal_eager_step()


def _graph_replays_equal_eager_step():
    sd, x, g, _, _, _ = _reference(1, 40, 512, 8, 4, 13)
    gru = _device_gru(1, 40, 512, sd)
    flat = FlatParams(gru.parameters())
    opt = Adam(gru.parameters(), lr=1e-3, flat=flat)
    xs, gs = x.cuda(), g.cuda()

    def body():
        opt.zero_grad()
        loss = (gru.forward_last(xs) * gs).sum()
        loss.backward()
        opt.step()
        return loss

    opt.sync_lr()   # lr lives in state_dev: written before the state is saved, so a restored state keeps it
    state = [flat.data, opt.exp_avg, opt.exp_avg_sq, opt.state_dev]
    start = [t.clone() for t in state]

    def from_start(fn):
        for t, s in zip(state, start):
            t.copy_(s)
        loss = fn()
        torch.cuda.synchronize()
        return [loss.detach().clone()] + [t.clone() for t in state]

    graph = GraphedStep(body, warmup=2)
    r1 = from_start(graph.replay)
    r2 = from_start(graph.replay)
    graph.release()
    eager = from_start(body)
    for a, b, c in zip(r1, r2, eager):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(r1[1], start[0])   # the step moved the parameters
    assert _lib.spin_timeouts() == 0


def test_top_last_entry_points_validate_on_the_host():
    """Null pointers and bad dimensions: a non-zero status and a message, before any device work (no GPU needed)."""
    L = _lib.lib()
    p = ctypes.c_void_p(256)
    mode = ctypes.c_int(0)

    def fwd(x=p, B=8, T=4, IN=40, H=512, y_last=p, m=ctypes.byref(mode)):
        return L.srk_gru_top_last_fwd(x, None, B, T, IN, H, p, p, p, p, p, y_last, p, m, None)

    def bwd(B=8, T=4, IN=40, H=512, dy_last=p, m=0, dw_hh=p):
        return L.srk_gru_top_last_bwd(p, None, B, T, IN, H, p, p, p, p, dy_last, m, None, p, dw_hh, p, p, 0, p, None)

    assert fwd(x=None) != 0 and b"null" in L.srk_last_error()
    assert fwd(y_last=None) != 0 and b"null" in L.srk_last_error()
    assert fwd(m=None) != 0 and b"null" in L.srk_last_error()
    assert fwd(B=0) != 0 and b"positive" in L.srk_last_error()
    assert fwd(H=500) != 0 and b"multiple of 128" in L.srk_last_error()
    assert bwd(dy_last=None) != 0 and b"null" in L.srk_last_error()
    assert bwd(dw_hh=None) != 0 and b"null" in L.srk_last_error()
    assert bwd(T=-1) != 0 and b"positive" in L.srk_last_error()
    assert bwd(H=130) != 0 and b"multiple of 128" in L.srk_last_error()
    assert bwd(m=4) != 0 and b"mode" in L.srk_last_error()
    # the backward workspace holds the layer's own plus the [B][T][2H] gradient the recurrence reads
    base = L.srk_gru_workspace_floats(8, 4, 40, 512, 1)
    assert L.srk_gru_top_last_workspace_floats(8, 4, 40, 512, 1) >= base + 8 * 4 * 1024
    assert L.srk_gru_top_last_workspace_floats(8, 4, 40, 512, 0) == L.srk_gru_workspace_floats(8, 4, 40, 512, 0)
