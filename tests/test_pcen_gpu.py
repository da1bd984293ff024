"""PCEN on the GPU: srk_pcen_fwd / _bwd against the float64 statement of tests/pcen_oracle.py, their determinism
under eager runs and a replayed graph, nn.PCEN, and the fbanks_cnn_pcen plugin (model parity in float64, 16-bit
matmul precision, warm start, graphed train steps through training.py).

Bound of the kernel parity, per case and per quantity: 4 x the error of the SAME statement evaluated in float32 on
the CPU against float64, with a floor of 1e-5 (the attention-pool kernels' bound).  The factor 4 allows for the
device's exp / log and another summation order.  y, M and dx are compared in max-norm over every element (relative
to the reference's largest element), dp per row in L2.  Measured on an MI355X (worst case of each quantity over the
cases, kernel / float32 CPU statement): y 2.3e-6 / 4.9e-7, M 8.4e-7 / 8.4e-7, dx 3.2e-6 / 1.0e-6, dp 3.3e-6 /
4.3e-6 (rows); the plugin's gradients against float64: 9.4e-4 norm-wise at batch 4 (pcen.params), 1.0e-6 at batch 2
(bound 2e-3)."""
import functools

import numpy as np
import pytest
import torch

from oracle import models as OM
from pcen_oracle import CASES, FbanksCnnPcen, errors, pcen_case, pcen_case_f32
from tolerances import LOGITS_REL, LOGITS_REL_LOWPREC, rel_err
from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import features as K
from speechrecognitionproject_amd import nn as snn
from speechrecognitionproject_amd.features import ptr, stream_ptr
from speechrecognitionproject_amd.graphs import GraphedStep
from speechrecognitionproject_amd.models import model_fbanks_cnn, model_fbanks_cnn_pcen
from speechrecognitionproject_amd.optim import Adam, FlatParams
from speechrecognitionproject_amd.synthetic import synthetic_clips

pytestmark = pytest.mark.gpu

GPU_CASES = ["1x1x1", "2x2x3", "5x7x64", "3x98x120", "4x130x65", "2x1024x1", "1x3x1024", "3x9x5lin"]
FLOOR, FACTOR = 1e-5, 4.0


def _device_inputs(name):
    c = pcen_case(name)
    return tuple(c[k].float().cuda() for k in ("x", "p", "dy"))


def _raw(name, x, p, dy, want_m=True, want_dx=True):
    """The two entry points on device tensors: {"y", "M", "dx", "dp"} (M / dx None when not asked for; the backward
    always reads an M a forward wrote)."""
    c = pcen_case(name)
    B, T, C = x.shape
    k, eps = c["log_scale"], c["eps"]
    y, m = torch.empty_like(x), torch.empty_like(x)
    dx = torch.empty_like(x) if want_dx else None
    dp = torch.empty_like(p)
    ws = torch.empty(int(_lib.lib().srk_pcen_workspace_floats(B, T, C)), device="cuda")
    _lib.call("srk_pcen_fwd", ptr(x), ptr(p), B, T, C, k, eps, ptr(y), ptr(m), stream_ptr())
    if not want_m:   # the evaluation form: the same forward without the write of M
        y = torch.empty_like(x)
        _lib.call("srk_pcen_fwd", ptr(x), ptr(p), B, T, C, k, eps, ptr(y), None, stream_ptr())
    _lib.call("srk_pcen_bwd", ptr(x), ptr(p), ptr(m), ptr(dy), B, T, C, k, eps, ptr(dx) if want_dx else None, ptr(dp),
              ptr(ws), stream_ptr())
    return {"y": y, "M": m if want_m else None, "dx": dx, "dp": dp}


def _bounds(name):
    f32 = errors(pcen_case_f32(name), pcen_case(name))
    return f32, {k: max(FLOOR, FACTOR * e) for k, e in f32.items()}


@pytest.mark.parametrize("name", GPU_CASES)
def test_pcen_vs_float64(gpu, name):
    c = pcen_case(name)
    B, T, C = CASES[name][:3]
    x, p, dy = _device_inputs(name)
    try:
        _lib.prof_enable(1)
        out = _raw(name, x, p, dy)
        torch.cuda.synchronize()
        kernels = [k for k in _lib.prof_kernels() if k["name"] == "pcen"]
        n, _, nbytes = _lib.prof_read("pcen")
    finally:
        _lib.prof_enable(0)
    for k, v in out.items():   # silent and step clips included
        assert torch.isfinite(v).all(), k
    got = errors({k: v.cpu() for k, v in out.items()}, c)
    f32, bound = _bounds(name)
    print("pcen %s: %s" % (name, "  ".join("%s %.2e (float32 CPU %.2e, bound %.2e)" % (k, got[k], f32[k], bound[k])
                                            for k in ("y", "M", "dx", "dp"))))
    for k in got:
        assert got[k] <= bound[k], (name, k, got[k], bound[k])
    if T == 1:   # no recurrence: M is E and no gradient reaches s
        assert torch.equal(out["dp"][3], torch.zeros_like(out["dp"][3]))
    # one launch forward, two backward (the scan, the parameter reduction), each with its byte count
    n_el = B * T * C
    assert n == 3 and nbytes == 4.0 * (3 * n_el + 4 * C) + 4.0 * (4 * n_el + 4 * C + 4 * B * C) + 4.0 * (4 * B * C + 8 * C)
    assert sum(k["launches"] for k in kernels) == 3 and all(k["bytes"] > 0 for k in kernels), kernels
    assert sorted(k["kernel"].split("<")[0].split(" ")[0] for k in kernels) == ["pcen_bwd_kernel", "pcen_dp_kernel",
                                                                               "pcen_fwd_kernel"]


@pytest.mark.parametrize("name", ["3x98x120", "4x130x65", "3x9x5lin", "1x1x1"])
def test_pcen_optional_outputs_do_not_change_the_others(gpu, name):
    """dx = NULL gives bitwise the same dp, m_out = NULL bitwise the same y."""
    x, p, dy = _device_inputs(name)
    full = _raw(name, x, p, dy)
    lean = _raw(name, x, p, dy, want_m=False, want_dx=False)
    assert lean["M"] is None and lean["dx"] is None
    assert torch.equal(full["y"], lean["y"]) and torch.equal(full["dp"], lean["dp"])


def test_pcen_is_deterministic_and_capturable(gpu):
    """Two eager runs give the same bits, and so do three replays of a captured forward + backward."""
    name = "3x98x120"
    x, p, dy = _device_inputs(name)
    first = {k: v.clone() for k, v in _raw(name, x, p, dy).items()}
    second = _raw(name, x, p, dy)
    for k in first:
        assert torch.equal(first[k], second[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _raw(name, x, p, dy)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _raw(name, x, p, dy)
    for _ in range(3):
        for o in outs.values():
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in first:
            assert torch.equal(first[k], outs[k]), k


def test_pcen_module_autograd(gpu):
    """nn.PCEN: the gradients of params and of a requires_grad input are the entry points' (so within the parity
    bounds of the oracle); under no_grad nothing is saved and no M buffer is allocated."""
    name = "5x7x64"
    c = pcen_case(name)
    x, p, dy = _device_inputs(name)
    raw = _raw(name, x, p, dy)
    mod = snn.PCEN(64).cuda()
    with torch.no_grad():
        mod.params.copy_(p)
    xm = x.clone().requires_grad_(True)
    y = mod(xm)
    (y * dy).sum().backward()
    assert torch.equal(y.detach(), raw["y"]) and torch.equal(xm.grad, raw["dx"]) and torch.equal(mod.params.grad, raw["dp"])
    got = errors({"y": y.detach().cpu(), "M": c["M"], "dx": xm.grad.cpu(), "dp": mod.params.grad.cpu()}, c)
    _, bound = _bounds(name)
    assert all(got[k] <= bound[k] for k in got), (got, bound)
    # an input without a gradient: the same dp, no dx
    mod.params.grad = None
    y2 = mod(x)
    (y2 * dy).sum().backward()
    assert torch.equal(mod.params.grad, raw["dp"])
    # linear mode through the module
    lin = pcen_case("3x9x5lin")
    ml = snn.PCEN(5, log_scale=0.0).cuda()
    with torch.no_grad():
        ml.params.copy_(lin["p"].float())
    assert rel_err(ml(lin["x"].float().cuda()).detach().cpu().numpy(), lin["y"].numpy()) <= 1e-5
    # evaluation: y only.  The forward's allocations are y (and M when a backward may follow)
    big = torch.rand(8, 98, 120, device="cuda") * 100 + 50
    mod120 = snn.PCEN(120).cuda()
    nbytes = big.numel() * 4

    def grown(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated() - before, out

    with torch.no_grad():
        mod120(big)   # nothing left to cache
        eval_bytes, ye = grown(lambda: mod120(big))
    assert ye.grad_fn is None and not ye.requires_grad
    assert nbytes <= eval_bytes < nbytes + 4096
    mod120(big)       # the cached workspace
    train_bytes, yt = grown(lambda: mod120(big))
    assert yt.grad_fn is not None and len(yt.grad_fn.saved_tensors) == 3
    assert 2 * nbytes <= train_bytes < 2 * nbytes + 8192
    assert torch.equal(ye, yt.detach())
    with pytest.raises(_lib.SrkError):
        mod120(big[:, :, :64])


# ----------------------------------------------------------------------------- the plugin
@functools.lru_cache(maxsize=None)
def _seeded():
    """fbanks_cnn's seeded weights plus front-end constants moved off their defaults (so that every row of
    pcen.params matters to the comparison)."""
    sd = OM.seeded_state_dict(FbanksCnnPcen(), 0)
    g = torch.Generator().manual_seed(5)
    sd["pcen.params"] = sd["pcen.params"] + 0.1 * torch.randn(4, 120, generator=g)
    return sd


def _features(x):
    with torch.no_grad():
        return K.fbank(torch.from_numpy(x).cuda()).cpu()


def _normwise(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("B", [4, 2])
def test_fbanks_cnn_pcen_vs_float64(gpu, B):
    """The model half (the oracle in float64 fed the HIP filter banks, which tests/test_features_gpu.py holds to
    their own tolerance): eval logits, then a train step with an injected dropout mask — loss, logits, and every
    gradient tensor norm-wise, pcen.params among them."""
    x, lab = synthetic_clips(B, seed=31 + B)
    sd = _seeded()
    net = model_fbanks_cnn_pcen.Network().cuda()
    assert set(net.state_dict()) == set(sd)
    net.load_state_dict(sd)                      # strict, both ways
    ref = FbanksCnnPcen()
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ref = ref.double()
    feats = _features(x)

    net.eval()
    ref.eval()
    with torch.no_grad():
        out = net(torch.from_numpy(x).cuda()).cpu().numpy()
        want = ref.forward_features(feats).numpy()
    assert rel_err(out, want) <= LOGITS_REL, rel_err(out, want)

    keep = (np.random.default_rng(44 + B).random((B, 512)) >= 0.5).astype(np.uint8)
    net.train()
    ref.train()
    net.dropout.set_mask(torch.from_numpy(keep))
    ref.dropout = OM.MaskDropout(keep)
    out = net(torch.from_numpy(x).cuda())
    loss = snn.CrossEntropyLoss()(out, torch.from_numpy(lab).cuda())
    loss.backward()
    rout = ref.forward_features(feats)
    rloss = torch.nn.CrossEntropyLoss()(rout, torch.from_numpy(lab))
    rloss.backward()
    assert rel_err(out.detach().cpu().numpy(), rout.detach().numpy()) <= LOGITS_REL
    assert abs(loss.item() - rloss.item()) <= 1e-4 * max(1.0, abs(rloss.item()))
    rgrads = dict(ref.named_parameters())
    names = [k for k, _ in net.named_parameters()]
    assert "pcen.params" in names
    worst = ("", 0.0)
    for k, q in net.named_parameters():
        assert q.grad is not None, k
        e = _normwise(q.grad.cpu().numpy(), rgrads[k].grad.numpy())
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= 2e-3, (k, e)
    print("fbanks_cnn_pcen B=%d: worst gradient norm-wise error %s %.3g; pcen.params %.3g"
          % (B, worst[0], worst[1], _normwise(net.pcen.params.grad.cpu().numpy(), rgrads["pcen.params"].grad.numpy())))


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fbanks_cnn_pcen_lowprec_logits(gpu, precision):
    x, _ = synthetic_clips(4, seed=37)
    net = model_fbanks_cnn_pcen.Network().cuda().eval()
    net.load_state_dict(_seeded())
    ref = FbanksCnnPcen().eval()
    ref.load_state_dict(_seeded())
    with torch.no_grad():
        want = ref.forward_features(_features(x)).numpy()
        try:
            _lib.set_matmul_precision(precision)
            _lib.prof_enable(1)
            out = net(torch.from_numpy(x).cuda()).cpu().numpy()
            n_pcen = _lib.prof_read("pcen")[0]
        finally:
            _lib.prof_enable(0)
            _lib.set_matmul_precision("fp32")
    assert n_pcen == 1   # fp32 at every matmul precision, and no M in evaluation
    assert rel_err(out, want) <= LOGITS_REL_LOWPREC, rel_err(out, want)


def test_fbanks_cnn_pcen_warm_starts_from_fbanks_cnn(gpu):
    """A fbanks_cnn checkpoint loads with strict=False: everything but the front-end."""
    sd = model_fbanks_cnn.Network().state_dict()
    res = model_fbanks_cnn_pcen.Network().load_state_dict(sd, strict=False)
    assert res.missing_keys == ["pcen.params"] and not res.unexpected_keys


def _train_setup(B, vtlp, seed):
    torch.manual_seed(0)
    net = model_fbanks_cnn_pcen.Network(vtlp=vtlp).cuda().train()
    net.load_state_dict(_seeded())
    flat = FlatParams(net.parameters())
    opt = Adam(net.parameters(), lr=1e-3, flat=flat)
    crit = snn.CrossEntropyLoss()
    x, lab = synthetic_clips(B, seed=seed)
    sx, sy = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()

    def body():
        opt.zero_grad()
        loss = crit(net(sx), sy)
        loss.backward()
        opt.step()
        return loss

    return net, body


def test_fbanks_cnn_pcen_vtlp_trains_one_step(gpu):
    """Network(vtlp=(0.9, 1.1)): one eager training step with the warped filter banks moves the front-end."""
    net, body = _train_setup(4, (0.9, 1.1), seed=41)
    before = net.pcen.params.detach().clone()
    loss = body().item()
    assert np.isfinite(loss) and float(net.pcen.params.grad.abs().max()) > 0
    assert bool(((net.last_alpha >= 0.9) & (net.last_alpha < 1.1)).all())
    assert not torch.equal(before, net.pcen.params.detach()) and torch.isfinite(net.pcen.params).all()


def test_fbanks_cnn_pcen_graph_replays_step_the_front_end(gpu):
    """pcen.params gets its gradient inside the captured backward and the fused Adam steps it: every replay moves
    it.  (No step runs on the capturing model before GraphedStep's own side-stream warm-up: a live autograd graph
    of a default-stream step would carry its AccumulateGrad nodes into the capture, graphs.py.)"""
    net, body = _train_setup(4, None, seed=43)
    g = GraphedStep(body, warmup=2)
    try:
        for _ in range(2):
            before = net.pcen.params.detach().clone()
            assert np.isfinite(g.replay().item())
            assert not torch.equal(before, net.pcen.params.detach())
            assert torch.isfinite(net.pcen.params).all()
    finally:
        g.release()


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_fbanks_cnn_pcen_training_entry_point(gpu, tmp_path, precision):
    from speechrecognitionproject_amd.training import main
    main(["-key", "t", "-lr", "0.001", "--model", "fbanks_cnn_pcen", "--synthetic", "64", "--batch-size", "16",
          "--precision", precision, "--output-path", str(tmp_path), "--log-every", "2", "--no-eval", "--save-model"])
    losses = [float(l) for l in open(tmp_path / "loss_t.txt")]
    assert len(losses) == 4 and all(np.isfinite(losses))   # two eager steps, the capture, two replays
    sd = torch.load(tmp_path / "models" / "model_t.ckpt", map_location="cpu")
    start = snn.PCEN(120).params.detach()
    assert torch.isfinite(sd["pcen.params"]).all()
    moved = (sd["pcen.params"] - start).abs() > 0
    assert bool(moved.any(dim=1).all()) and float(moved.float().mean()) > 0.9   # Adam stepped all four rows
