"""The data gradient of the fused conv1 + max-pool layer (srk_conv1_pool_dgrad), which an input with a gradient
needs (a trainable front-end before conv1: model_fbanks_cnn_pcen).

The reference is float64 autograd of torch's CPU conv2d on the same weights, fed the pooled gradient unpooled
through THE KERNEL'S OWN argmax (so a near tie in a pool window, which float32 and float64 may break differently,
does not enter: the forward and its argmax are tests/test_conv_gpu.py's subject).  Bound: 1e-5 of the largest
element, the project's fp32 kernel bound (tests/test_dconv_gpu.py) — each element is a sum of 64 x 21 products in
float32, about sqrt(1344) x 6e-8 = 2e-6 of the scale."""
import pytest
import torch

from tolerances import rel_err
from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import nn as snn
from speechrecognitionproject_amd.features import ptr, stream_ptr

pytestmark = pytest.mark.gpu

FB = (7, 3, 3, 1, 3)     # KH, KW, ph, pw, pool: model_fbanks_cnn
SC = (3, 7, 1, 3, 5)     # model_spec_cnn
CASES = [(3, 98, 120) + FB,      # the plugin's image
         (2, 7, 9) + FB,         # fewer rows than taps, three windows
         (1, 5, 3) + FB,         # one window: no neighbours
         (2, 19, 33) + FB,       # more than one row block, a short last one
         (2, 9, 35) + SC, (1, 49, 320) + SC]


def _case(N, H, W, KH, KW, ph, pw, pool):
    g = torch.Generator().manual_seed(100 * N + 10 * H + W)
    x = torch.randn(N, H, W, generator=g)
    w = torch.randn(64, 1, KH, KW, generator=g) * (KH * KW) ** -0.5
    b = torch.randn(64, generator=g)
    dy = torch.randn(N, H, W // pool, 64, generator=g)
    return x, w, b, dy


@pytest.mark.parametrize("case", CASES)
def test_conv1_pool_dgrad_vs_float64(gpu, case):
    N, H, W, KH, KW, ph, pw, pool = case
    x, w, b, dy = _case(*case)
    xd, wd, bd, dyd = (t.cuda() for t in (x, w, b, dy))
    y = torch.empty(N, H, W // pool, 64, device="cuda")
    arg = torch.empty(N, H, W // pool, 64, device="cuda", dtype=torch.uint8)
    dx = torch.full((N, H, W), float("nan"), device="cuda")
    _lib.call("srk_conv1_pool_fwd", ptr(xd), N, H, W, ptr(wd), ptr(bd), 64, KH, KW, ph, pw, pool, ptr(y), ptr(arg),
              stream_ptr())
    try:
        _lib.prof_enable(1)
        _lib.call("srk_conv1_pool_dgrad", ptr(wd), N, H, W, 64, KH, KW, ph, pw, pool, ptr(dyd), ptr(arg), ptr(dx),
                  stream_ptr())
        torch.cuda.synchronize()
        n, _, nbytes = _lib.prof_read("conv1_pool_dgrad")
    finally:
        _lib.prof_enable(0)
    assert n == 1 and nbytes == 4.0 * N * H * W + 5.0 * N * H * (W // pool) * 64
    # the pooled gradient at the kernel's argmax, as the dense gradient of the conv output [N, 64, H, W]
    a = arg.cpu().long()
    assert int(a.max()) < pool
    dU = torch.zeros(N, H, W // pool, pool, 64, dtype=torch.float64)
    dU.scatter_(3, a.unsqueeze(3), dy.double().unsqueeze(3))
    dU = dU.reshape(N, H, W, 64).permute(0, 3, 1, 2)
    x64 = x.double().unsqueeze(1).requires_grad_(True)
    torch.nn.functional.conv2d(x64, w.double(), b.double(), padding=(ph, pw)).backward(dU)
    err = rel_err(dx.cpu().numpy(), x64.grad[:, 0].numpy())
    print("conv1_pool_dgrad %s: %.2e" % (case, err))
    assert torch.isfinite(dx).all() and err <= 1e-5, err
    again = torch.empty_like(dx)
    _lib.call("srk_conv1_pool_dgrad", ptr(wd), N, H, W, 64, KH, KW, ph, pw, pool, ptr(dyd), ptr(arg), ptr(again),
              stream_ptr())
    assert torch.equal(dx, again)   # fixed summation order


def test_conv1_pool_autograd_returns_the_input_gradient(gpu):
    """nn.conv1_pool on an input with a gradient stays on the fused kernels and hands back srk_conv1_pool_dgrad's
    result; the weight and bias gradients are the ones an input without a gradient gets."""
    N, H, W = 2, 19, 33
    x, w, b, dy = _case(N, H, W, *FB)
    conv, pool = snn.Conv2d(1, 64, kernel_size=(7, 3), padding=(3, 1)).cuda(), snn.MaxPool2d((1, 3))
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    grads = []
    for needs in (True, False):
        conv.weight.grad = conv.bias.grad = None
        xd = x.cuda().requires_grad_(needs)
        try:
            _lib.prof_enable(1)
            y = snn.conv1_pool(xd, conv, pool)
            (y * dy.cuda()).sum().backward()
            torch.cuda.synchronize()
            counts = [_lib.prof_read(k)[0] for k in ("conv1_pool_fwd", "conv1_pool_wgrad", "conv1_pool_dgrad")]
        finally:
            _lib.prof_enable(0)
        assert counts == [1, 1, 1 if needs else 0]
        grads.append((xd.grad, conv.weight.grad.clone(), conv.bias.grad.clone()))
    assert grads[0][0] is not None and grads[1][0] is None
    assert torch.equal(grads[0][1], grads[1][1]) and torch.equal(grads[0][2], grads[1][2])
    x64 = x.double().unsqueeze(1).requires_grad_(True)
    ref = torch.nn.functional.max_pool2d(torch.nn.functional.conv2d(x64, w.double(), b.double(), padding=(3, 1)), (1, 3))
    ref.backward(dy.double().permute(0, 3, 1, 2))
    assert rel_err(grads[0][0].cpu().numpy(), x64.grad[:, 0].numpy()) <= 1e-5


def test_conv1_pool_dgrad_rejects_a_width_the_windows_do_not_cover(gpu):
    N, H, W = 1, 5, 10
    z = torch.zeros(N, H, W, device="cuda")
    w = torch.zeros(64, 1, 7, 3, device="cuda")
    dy = torch.zeros(N, H, 3, 64, device="cuda")
    arg = torch.zeros(N, H, 3, 64, device="cuda", dtype=torch.uint8)
    with pytest.raises(_lib.SrkError, match="conv1_pool_dgrad"):
        _lib.call("srk_conv1_pool_dgrad", ptr(w), N, H, W, 64, 7, 3, 3, 1, 3, ptr(dy), ptr(arg), ptr(z), stream_ptr())
    with pytest.raises(_lib.SrkError, match="conv1_pool_dgrad"):
        _lib.call("srk_conv1_pool_dgrad", ptr(w), N, H, 9, 64, 7, 3, 3, 1, 3, ptr(dy), ptr(arg), None, stream_ptr())
