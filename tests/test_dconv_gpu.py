"""Dilated 1-D convolutions (srk_conv1d_nlc_dil_*, nn.Conv1d(dilation=)) vs torch on the CPU, and the
resnet_dconv plugin vs the fixture written from the reference (tests/golden/make_resnet_dconv_golden.py)."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import models as OM
from resnet_dconv_oracle import ResnetDconv, sampled_grad_errors
from tolerances import LOGITS_REL, rel_err
from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import nn as snn
from speechrecognitionproject_amd.graphs import GraphedStep
from speechrecognitionproject_amd.models import model_resnet_dconv
from speechrecognitionproject_amd.optim import Adam, FlatParams
from speechrecognitionproject_amd.synthetic import synthetic_clips

pytestmark = pytest.mark.gpu

CASES = [  # N, L, Ci, Co, K, pad, dil
    (2, 61, 64, 128, 5, 8, 4),       # ragged tile edge
    (3, 37, 32, 64, 5, 32, 16),      # receptive field 65 > L: the outer taps are mostly outside
    (2, 50, 5, 7, 3, 2, 2),          # channel counts that miss the vector gathers
    (2, 40, 24, 40, 4, 3, 3),        # even kernel, Lo = 37 != L
    (2, 33, 64, 64, 5, 0, 4),        # no padding, Lo = 17
    (8, 500, 64, 128, 5, 32, 16),    # many tiles, split-K weight gradient
    (2, 500, 384, 512, 5, 8, 4),     # model_resnet_dconv.py:99
    (2, 500, 512, 640, 5, 32, 16),   # model_resnet_dconv.py:100
]
MODEL_CASES = CASES[6:]
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs of a case and torch's CPU results (NCL layout), computed once and shared (never written to)."""
    N, L, Ci, Co, K, pad, dil = case
    g = torch.Generator().manual_seed(N * 100 + Co + dil)
    x = torch.randn(N, Ci, L, generator=g)
    w = torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    b = torch.randn(Co, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv1d(xr, wr, br, padding=pad, dilation=dil)
    assert yr.shape[2] == L + 2 * pad - dil * (K - 1)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    return x, w, b, gy, yr.detach(), xr.grad, wr.grad, br.grad


def _run_module(case, x, w, b, gy):
    """nn.Conv1d(dilation=) forward + backward on channels-last tensors: (y, dx, dw, db), all on the device."""
    N, L, Ci, Co, K, pad, dil = case
    conv = snn.Conv1d(Ci, Co, K, padding=pad, dilation=dil).cuda()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    xm = x.transpose(1, 2).contiguous().cuda().requires_grad_(True)
    ym = conv(xm)
    (ym * gy.transpose(1, 2).cuda()).sum().backward()
    return ym.detach(), xm.grad, conv.weight.grad, conv.bias.grad


def _check_case(case):
    x, w, b, gy, yr, dxr, dwr, dbr = _case(case)
    y, dx, dw, db = _run_module(case, x, w, b, gy)
    assert y.transpose(1, 2).shape == yr.shape
    errs = (rel_err(y.transpose(1, 2).cpu().numpy(), yr.numpy()), rel_err(dx.transpose(1, 2).cpu().numpy(), dxr.numpy()),
            rel_err(dw.cpu().numpy(), dwr.numpy()), rel_err(db.cpu().numpy(), dbr.numpy()))
    print("dconv %s: y %.2e dx %.2e dw %.2e db %.2e" % ((case,) + errs))
    assert errs[0] <= 1e-5 and errs[1] <= 1e-5 and errs[2] <= 1e-4 and errs[3] <= 1e-5, errs


def _kernels():
    return " ".join(k["kernel"] for k in _lib.prof_kernels())


@pytest.mark.parametrize("case", CASES)
def test_dilated_conv1d_vs_torch(gpu, case):
    _check_case(case)


@pytest.mark.parametrize("case", MODEL_CASES)
def test_dilated_conv1d_ring_vs_torch(gpu, case):
    """conv_ring = 0x87: the fp32 LDS-DMA ring kernels at any K — the head's shapes qualify in all three modes
    (channel counts % 16, >= 128 output columns, stride 1), and the ring kernels take dilation."""
    try:
        with _lib.options(conv_ring=0x87):
            _lib.prof_enable(1)
            _check_case(case)
            torch.cuda.synchronize()
            ks = _kernels()
    finally:
        _lib.prof_enable(0)
    for mode in ("fwd", "dgrad", "wgrad"):
        assert "conv_ring_kernel<%s" % mode in ks, (mode, ks)


def test_dilation_1_equals_existing_path_bitwise(gpu):
    """srk_conv1d_nlc_dil_* at dil = 1 forward to srk_conv2d_nhwc_fwd16 / _bwd16_acc: the same bits."""
    N, L, Ci, Co, K, pad = 2, 61, 64, 128, 5, 2
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, L, Ci, generator=g).cuda()
    w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).cuda()
    b = torch.randn(Co, generator=g).cuda()
    gy = torch.randn(N, L + 2 * pad - (K - 1), Co, generator=g).cuda()
    outs = []
    for dilated in (False, True):
        xm, wm, bm = (t.clone().requires_grad_(True) for t in (x, w, b))
        if dilated:
            ym = snn._Conv1dDilFn.apply(xm, wm, bm, pad, 1)
        else:
            ym = snn._Conv2dNHWCFn.apply(xm.reshape(N, 1, L, Ci), wm, bm, (0, pad), (1, 1)).reshape(N, -1, Co)
        (ym * gy).sum().backward()
        outs.append((ym.detach(), xm.grad, wm.grad, bm.grad))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    # and nn.Conv1d's default is that path
    conv = snn.Conv1d(Ci, Co, K, padding=pad).cuda()
    assert conv.dilation == (1,)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    assert torch.equal(conv(x).detach(), outs[0][0])


@pytest.mark.parametrize("case", [CASES[1], CASES[2]])
def test_dilated_conv1d_no_leak_across_clips(gpu, case):
    """N = 3 with clip 1 all NaN (x for the forward, dY for the data gradient): the neighbouring clips stay finite
    and bitwise what they are with clip 1 zero — no tap reads across a clip boundary."""
    _, L, Ci, Co, K, pad, dil = case
    N = 3
    g = torch.Generator().manual_seed(Ci + dil)
    x = torch.randn(N, L, Ci, generator=g)
    w = (torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5).cuda()
    b = torch.randn(Co, generator=g).cuda()
    gy = torch.randn(N, L + 2 * pad - dil * (K - 1), Co, generator=g)
    res = {}
    for tag, fill in (("zero", 0.0), ("nan", float("nan"))):
        x1, gy1 = x.clone(), gy.clone()
        x1[1] = fill
        xm = x1.cuda().requires_grad_(True)
        y = snn.conv1d_nlc(xm, w, b, 1, pad, dil)
        res["y", tag] = y.detach().clone()
        gy1[1] = fill
        xm2 = x.cuda().requires_grad_(True)
        (snn.conv1d_nlc(xm2, w, b, 1, pad, dil) * gy1.cuda()).sum().backward()
        res["dx", tag] = xm2.grad.clone()
    for what in ("y", "dx"):
        bad, zero = res[what, "nan"], res[what, "zero"]
        for clip in (0, 2):
            assert torch.isfinite(bad[clip]).all(), (what, clip)
            assert torch.equal(bad[clip], zero[clip]), (what, clip)
        assert torch.isnan(bad[1]).any()


@pytest.fixture(params=["bf16", "fp16"])
def prec(request, gpu):
    _lib.set_matmul_precision(request.param)
    yield request.param
    _lib.set_matmul_precision("fp32")


@functools.lru_cache(maxsize=None)
def _case_rounded(case, prec):
    """float64 convolutions of the host-rounded operands (x, w for fwd; dy, w for dgrad; x, dy for wgrad)."""
    N, L, Ci, Co, K, pad, dil = case
    x, w, b, gy = _case(case)[:4]
    xr, wr, gr = (t.to(TORCH_DT[prec]).double() for t in (x, w, gy))
    y_ref = F.conv1d(xr, wr, b.double(), padding=pad, dilation=dil)
    dx_ref = torch.nn.grad.conv1d_input(x.shape, wr, gr, padding=pad, dilation=dil)
    dw_ref = torch.nn.grad.conv1d_weight(xr, w.shape, gr, padding=pad, dilation=dil)
    return y_ref, dx_ref, dw_ref


@pytest.mark.parametrize("case", [c for c in CASES if c[2] % 8 == 0 and c[3] % 8 == 0])
def test_dilated_conv1d_lowprec_exact_rounding(prec, case):
    """16-bit operands: == the float64 convolution of the host-rounded operands up to fp32 summation order."""
    N, L, Ci, Co, K, pad, dil = case
    x, w, b, gy = _case(case)[:4]
    y_ref, dx_ref, dw_ref = _case_rounded(case, prec)
    try:
        _lib.prof_enable(1)
        y, dx, dw, _ = _run_module(case, x, w, b, gy)
        torch.cuda.synchronize()
        n_lp = [_lib.prof_read(c)[0] for c in ("conv_fwd_lp", "conv_dgrad_lp", "conv_wgrad_lp")]
        ks = _kernels()
    finally:
        _lib.prof_enable(0)
    assert min(n_lp) >= 1, "the 16-bit conv kernels did not run: %s" % n_lp
    if case in MODEL_CASES:   # channel counts % 32: the 16-bit LDS-DMA ring in every mode
        for mode in ("fwd", "dgrad", "wgrad"):
            assert "conv_ring16_kernel<%s" % mode in ks, (mode, ks)

    def close(out, ref, k):
        # fp32 accumulation of k rounded products; only the summation order differs
        err, bound = (out.double() - ref).abs().max().item(), 1e-5 * (1 + ref.abs().max().item()) * max(1.0, (k / 256) ** 0.5)
        print("dconv %s %s: err %.3g bound %.3g" % (case, prec, err, bound))
        return err <= bound

    assert close(y.transpose(1, 2).cpu(), y_ref, Ci * K)
    assert close(dx.transpose(1, 2).cpu(), dx_ref, Co * K)
    assert close(dw.cpu(), dw_ref, N * y_ref.shape[2])


# ----------------------------------------------------------------------------- the plugin vs the reference fixture
@pytest.fixture(scope="module")
def fixture():
    return golden("resnet_dconv_golden.npz")


def _plugin_step(g, train_mode):
    net = model_resnet_dconv.Network().cuda()
    net.load_state_dict(OM.seeded_state_dict(ResnetDconv(), 0))
    net.train(train_mode)
    params = dict(net.named_parameters())
    before = {k: v.detach().clone() for k, v in params.items()}
    opt = Adam(net.parameters(), lr=1e-4)
    opt.zero_grad()
    out = net(torch.from_numpy(g["pcm"]))
    loss = snn.CrossEntropyLoss()(out, torch.from_numpy(g["labels"]).cuda())
    loss.backward()
    grads = {k: v.grad.detach().clone() for k, v in params.items()}
    opt.step()
    return net, params, before, out.detach().cpu().numpy(), loss.item(), grads


def test_resnet_dconv_eval_record(gpu, fixture):
    """Eval mode (BatchNorm on running statistics; the reference's float32 and float64 agree to 2e-6): the tight
    record.  Sampled gradients vs float64 <= 2e-3 max-norm per tensor, first-step Adam deltas >= 98 % within 2e-6."""
    g = fixture
    net, params, before, out, loss, grads = _plugin_step(g, False)
    assert rel_err(out, g["ev_logits64"]) <= LOGITS_REL
    assert abs(loss - float(g["ev_loss64"])) <= 1e-4 * max(1.0, abs(float(g["ev_loss64"])))
    worst = ("", 0.0)
    fails = []
    for k in g["names"]:
        idx = g["ev_gidx__" + k]
        mx, _ = sampled_grad_errors(grads[k].cpu().numpy(), idx, g["ev_g64__" + k])
        worst = max(worst, (k, mx), key=lambda t: t[1])
        if mx > 2e-3:
            fails.append((k, mx))
        dv = (params[k].detach() - before[k]).reshape(-1).cpu().numpy()[idx]
        # Adam's first step is ~lr*sign(g): entries whose grad is ~0 may flip sign
        assert np.mean(np.abs(dv - g["ev_dval__" + k]) <= 2e-6) >= 0.98, k
    print("resnet_dconv eval: worst sampled-gradient max-norm error %s %.3g" % worst)
    assert not fails, fails


def test_resnet_dconv_train_record(gpu, fixture):
    """Train mode: logits, loss and running statistics as tight as eval; gradients normwise over the sampled entries
    vs float64 <= 5e-2 per tensor (4 x the reference's own worst float32 value, 1.2e-2: a single ReLU sign flip
    between two roundings moves whole tensors here, so this check is coarse on purpose)."""
    g = fixture
    net, params, before, out, loss, grads = _plugin_step(g, True)
    assert rel_err(out, g["tr_logits64"]) <= LOGITS_REL
    assert abs(loss - float(g["tr_loss64"])) <= 1e-4 * max(1.0, abs(float(g["tr_loss64"])))
    sd = net.state_dict()
    n_stats = 0
    for key in g.files:
        if key.startswith("tr_stat64__"):
            assert rel_err(sd[key[len("tr_stat64__"):]].cpu().numpy(), g[key]) <= LOGITS_REL, key
            n_stats += 1
    assert n_stats == 2 * 20   # 17 BatchNorms in blocks / stem + 3 downsample ones
    worst = ("", 0.0)
    fails = []
    for k in g["names"]:
        _, nrm = sampled_grad_errors(grads[k].cpu().numpy(), g["tr_gidx__" + k], g["tr_g64__" + k])
        worst = max(worst, (k, nrm), key=lambda t: t[1])
        if nrm > 5e-2:
            fails.append((k, nrm))
    print("resnet_dconv train: worst sampled-gradient normwise error %s %.3g (reference float32: %.3g)"
          % (worst + (float(g["tr_ref32_norm_err"]),)))
    assert not fails, fails


def test_resnet_dconv_state_dict_layout(gpu, fixture):
    net = model_resnet_dconv.Network()
    sd = net.state_dict()
    assert list(sd.keys()) == list(fixture["sd_keys"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(fixture["sd_shapes"])
    net.load_state_dict(ResnetDconv().state_dict())   # strict: a state dict saved from the restatement loads


def _setup(B, seed):
    net = model_resnet_dconv.Network().cuda()
    net.load_state_dict(OM.seeded_state_dict(ResnetDconv(), 0))
    net.train()
    flat = FlatParams(net.parameters())
    opt = Adam(net.parameters(), lr=1e-4, flat=flat)
    x, y = synthetic_clips(3 * B, seed=seed)
    return net, flat, opt, torch.from_numpy(x).cuda().view(3, B, -1), torch.from_numpy(y).cuda().view(3, B)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_resnet_dconv_graph_replay_equals_eager_steps(gpu, precision):
    """K train steps replayed from one captured HIP graph == the same steps run eagerly, bit for bit (parameters,
    Adam moments, device step count, BatchNorm running statistics, losses)."""
    K, B = 4, 4
    try:
        _lib.set_matmul_precision(precision)
        states = []
        for graphed in (False, True):
            torch.manual_seed(0)
            net, flat, opt, pcm, lab = _setup(B, seed=17)
            crit = snn.CrossEntropyLoss()
            sx, sy = pcm[0].clone(), lab[0].clone()

            def body():
                opt.zero_grad()
                loss = crit(net(sx), sy)
                loss.backward()
                opt.step()
                return loss

            losses = []
            if graphed:
                with warnings.catch_warnings(record=True) as ws:
                    warnings.simplefilter("always")
                    g = GraphedStep(body, warmup=2)         # 2 eager steps on batch 0, then the capture
                    for i in range(K):
                        sx.copy_(pcm[(i + 1) % 3])
                        sy.copy_(lab[(i + 1) % 3])
                        losses.append(g.replay().item())
                bad = [str(w.message)[:120] for w in ws if "AccumulateGrad" in str(w.message)]
                assert not bad, bad
                g.release()
            else:
                for i in range(2 + K):
                    if i >= 2:
                        sx.copy_(pcm[(i - 1) % 3])
                        sy.copy_(lab[(i - 1) % 3])
                    loss = body()
                    if i >= 2:
                        losses.append(loss.item())
            torch.cuda.synchronize()
            bufs = [b.detach().clone() for n, b in net.named_buffers() if "running" in n]
            states.append((flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.state_dev.clone(),
                           bufs, losses))
    finally:
        _lib.set_matmul_precision("fp32")
    (p0, m0, v0, s0, b0, l0), (p1, m1, v1, s1, b1, l1) = states
    assert int(s0[0]) == int(s1[0]) == 2 + K
    assert all(np.isfinite(l0)) and l0 == l1
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert all(torch.equal(a, b) for a, b in zip(b0, b1))


def test_resnet_dconv_training_entry_point(gpu, tmp_path):
    from speechrecognitionproject_amd.training import main
    main(["-key", "t", "-lr", "0.0001", "--model", "resnet_dconv", "--synthetic", "48", "--batch-size", "16",
          "--output-path", str(tmp_path), "--log-every", "2"])
    losses = [float(l) for l in open(tmp_path / "loss_t.txt")]
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert len(open(tmp_path / "val_t.txt").readlines()) == 1
    assert len(open(tmp_path / "train_t.txt").readlines()) == 1
