"""The clipped dx GEMM of the last-step top BiGRU layer (gru_top_last = 3, the default; csrc/gru.hip layer_bwd).

Where the full dx GEMM dgi [B T, 6H] x W_ih_cat [6H, in] plans as the stream-K ping-pong kernel, the backward runs it
through gemm_f32_klive: the reverse direction's 3H columns of dgi are zero in every row but the B rows (b, T-1), so
the K-tiles of that half are skipped with the cuts unmoved, the live rows are completed over the full K, and the zero
fill of those columns goes (with the grouped dW launch on, which reads none of them either).  Every element keeps the
full layer's bits, so forward_last is compared with last_step(forward(x)[0]) by torch.equal.

One layer, H = 512, in = 1022 (the padded path: dx comes out at width 1024 in a pad buffer, unpad_cols after it),
B = 161, T = 51: 33 x 4 = 132 tiles of 256 x 256 on 256 CUs, a stream-K plan, with a ragged last tile row and 5 - 6
live rows per tile.  The plan is confirmed by srk_gemm_plan_describe and the profiler records, so a silent fallback
cannot pass.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import nn as snn
from speechrecognitionproject_amd.graphs import GraphedStep
from speechrecognitionproject_amd.optim import Adam, FlatParams

import bigru_group_worker as W

H = W.H
IN, B, T = 1022, 161, 51


def _dx_plan():
    buf = ctypes.create_string_buffer(512)
    base = 1 << 20
    _lib.call("srk_gemm_plan_describe", 0, 0, B * T, 1024, 6 * H, 6 * H, 1024, 1024, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0,
              base, 2 * base, 3 * base, 0, buf, len(buf))
    return buf.value.decode().split("\n")[0]


def _profiled(fn):
    _lib.prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        kernels = [k["kernel"] for k in _lib.prof_kernels()]
    finally:
        _lib.prof_enable(0)
    return out, kernels


def _klive_records(kernels):
    clipped = [k for k in kernels if k.startswith("gemm_p32_kernel<NN> %dx1024x%d " % (B * T, 6 * H)) and
               k.endswith("streamk klive %d" % (3 * H))]
    rows = [k for k in kernels if k.startswith("p32_live_rows_kernel<NN> %dx1024x%d " % (B * T, 6 * H))]
    return clipped, rows


def _assert_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.fixture(scope="module")
def case():
    return W.inputs(IN, B, T)


@pytest.fixture(scope="module")
def last_step_results(gpu, case):
    """forward_last in this process (klive and the group on), with its profiler records."""
    sd, x, g = case
    return _profiled(lambda: W.run(W.device_gru(IN, sd), x, g, True))


@pytest.mark.gpu
def test_default_mode_has_the_full_layers_bits(gpu, case, last_step_results):
    plan = _dx_plan()
    assert "|gemm_p32_kernel<NN>" in plan and plan.endswith(" streamk"), plan
    sd, x, g = case
    full = W.run(W.device_gru(IN, sd), x, g, False)
    last, kernels = last_step_results
    clipped, rows = _klive_records(kernels)
    assert len(clipped) == 1 and len(rows) == 1, kernels
    _assert_equal(last, full)
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
def test_accumulating_backward_has_the_full_layers_bits(gpu, case):
    """accumulate = 1: gradients owned by FlatParams and pre-filled, two backward passes without zero_grad."""
    sd, x, g = case
    fill = torch.randn(sum(v.numel() for v in sd.values()) + 4096, generator=torch.Generator().manual_seed(5))

    def two_passes(last):
        gru = W.device_gru(IN, sd)
        flat = FlatParams(gru.parameters())
        flat.grad.copy_(fill[:flat.grad.numel()].cuda())
        xg = x.cuda().requires_grad_(True)
        for _ in range(2):
            y = gru.forward_last(xg) if last else snn.last_step(gru(xg)[0])
            (y * g.cuda()).sum().backward()
        torch.cuda.synchronize()
        return {"grad": flat.grad.clone(), "dx": xg.grad.clone()}

    full = two_passes(False)
    last, kernels = _profiled(lambda: two_passes(True))
    clipped, rows = _klive_records(kernels)
    assert len(clipped) == 1 and len(rows) == 1, kernels
    _assert_equal(last, full)
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["SRK_GEMM_KLIVE", "SRK_GEMM_GROUP"])
def test_switch_off_in_a_child_process_gives_the_same_bits(gpu, case, last_step_results, tmp_path, switch):
    """SRK_GEMM_KLIVE=0 keeps the full dx GEMM; SRK_GEMM_GROUP=0 keeps klive but also the zero fill (the full dW_ih
    GEMM reads it).  Both are read once per process, so a child computes the case; its bits are this process's."""
    out = str(tmp_path / "child.pt")
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, os.path.join(W.HERE, "bigru_group_worker.py"), str(IN), str(B), str(T), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = torch.load(out)
    last, _ = last_step_results
    _assert_equal({k: v.cpu() for k, v in last.items()}, child)


@pytest.mark.gpu
def test_graph_replays_equal_eager_step(gpu, case):
    """forward + backward + Adam captured with GraphedStep: two replays from the same state are bitwise equal to each
    other and to the eager step from that state (whose launches include the clipped dx)."""
    sd, x, g = case
    gru = W.device_gru(IN, sd)
    flat = FlatParams(gru.parameters())
    opt = Adam(gru.parameters(), lr=1e-3, flat=flat)
    xs, gs = x.cuda().requires_grad_(True), g.cuda()

    def body():
        opt.zero_grad()
        xs.grad = None
        loss = (gru.forward_last(xs) * gs).sum()
        loss.backward()
        opt.step()
        return loss, xs.grad

    opt.sync_lr()
    state = [flat.data, opt.exp_avg, opt.exp_avg_sq, opt.state_dev]
    start = [t.clone() for t in state]

    def from_start(fn):
        for t, s in zip(state, start):
            t.copy_(s)
        loss, dx = fn()
        torch.cuda.synchronize()
        return [loss.detach().clone(), dx.detach().clone()] + [t.clone() for t in state]

    graph = GraphedStep(body, warmup=2)
    r1 = from_start(graph.replay)
    r2 = from_start(graph.replay)
    graph.release()
    eager, kernels = _profiled(lambda: from_start(body))
    clipped, rows = _klive_records(kernels)
    assert len(clipped) == 1 and len(rows) == 1, kernels
    for a, b, c in zip(r1, r2, eager):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(r1[2], start[0])   # the step moved the parameters
    assert _lib.spin_timeouts() == 0
