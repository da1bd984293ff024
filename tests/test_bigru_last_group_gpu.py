"""The grouped dW launch of the last-step top BiGRU layer (gru_top_last = 3, the default; csrc/gru.hip layer_bwd).

Where the full dW_ih GEMM runs on gemm_p32_kernel with a K split and T >= 16, the backward issues one
gemm_p32_group launch for the dW_ih forward half, the forward dW_hh and the reverse half of dW_ih with its all-zero
8-deep k blocks deleted.  Every element keeps the accumulation order the full layer gives it, so forward_last is
compared with last_step(forward(x)[0]) by torch.equal on y_last, every gradient and dx.  One layer, H = 512,
in = 1024.  (B, T): the smallest at which the path engages (the full dW_ih splits from B T = 320: 48 tiles,
choose_splits with BK = 16), with T = 16 (the threshold), T = 17 and B T no multiple of 8, and 65 x 19 (a partial
64-row recurrence group, B T odd); every choice is confirmed against srk_gemm_plan_describe.  At (64, 8) the layer
must take the ungrouped launches (T < 16).  Each test reads srk_prof_kernels after an eager pass: the group record
is there in the first set and absent in the second, so a silent fallback cannot pass.
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
GROUPED = [(20, 16), (24, 17), (65, 19)]


def _describe(ta, tb, M, N, K, lda, ldb, ldc, batch=1, sA=0, sB=0, sC=0, rowsum=0, plan_batch=0):
    buf = ctypes.create_string_buffer(512)
    base = 1 << 20
    _lib.call("srk_gemm_plan_describe", ta, tb, M, N, K, lda, ldb, ldc, batch, sA, sB, sC, 0, rowsum, 0, 0, 0, plan_batch,
              base, 2 * base, 3 * base, 0, buf, len(buf))
    return buf.value.decode().split("\n")[0]


def _full_dw_plans(B, T, ld=1024):
    """The records of the full dW_ih GEMM and of the two-direction dW_hh launch at (B, T)."""
    BT = B * T
    ih = _describe(1, 0, 6 * H, ld, BT, 6 * H, ld, ld, rowsum=1)
    hh = _describe(1, 0, 3 * H, H, BT - 1, 3 * H, 2 * H, H, batch=2, sA=BT * 3 * H - 3 * H, sB=3 * H, sC=3 * H * H,
                   rowsum=1)
    return ih, hh


def _splits(record):
    return int(record.rsplit(" s", 1)[1].split()[0])


def _profiled(fn):
    """fn()'s result and the (kernel detail) records of its launches."""
    _lib.prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        kernels = [k["kernel"] for k in _lib.prof_kernels()]
    finally:
        _lib.prof_enable(0)
    return out, kernels


def _group_records(kernels):
    return [k for k in kernels if k.startswith(W.GROUP_RECORD)]


def _assert_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def _last_vs_full(IN, B, T):
    sd, x, g = W.inputs(IN, B, T)
    gru = W.device_gru(IN, sd)
    full = W.run(gru, x, g, False)
    last, kernels = _profiled(lambda: W.run(gru, x, g, True))
    _assert_equal(last, full)
    assert int(torch.count_nonzero(last["dweight_hh_l0_reverse"])) == 0
    return kernels


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", GROUPED)
def test_grouped_backward_has_the_full_layers_bits(gpu, B, T):
    ih, hh = _full_dw_plans(B, T)
    assert "|gemm_p32_kernel<TN>" in ih and _splits(ih) > 1, ih     # the path's conditions hold at this shape
    assert "|gemm_p32_kernel<TN>" in hh and " b2 " in hh, hh
    kernels = _last_vs_full(1024, B, T)
    recs = _group_records(kernels)
    assert len(recs) == 1, kernels
    # the members: the forward half on the full GEMM's split, the forward dW_hh on the two-direction launch's, the
    # packed reverse half (at least the B kept blocks, fewer rows than B T) on the full GEMM's split again
    members = recs[0].split()[1:]
    assert len(members) == 3
    assert "%dx1024x%ds%d" % (3 * H, B * T, _splits(ih)) in members
    assert "%dx%dx%ds%d" % (3 * H, H, B * T - 1, _splits(hh)) in members
    packed = [m for m in members if m.startswith("%dx1024x" % (3 * H)) and m != "%dx1024x%ds%d" % (3 * H, B * T, _splits(ih))]
    assert len(packed) == 1 and packed[0].endswith("s%d" % _splits(ih))
    kp = int(packed[0].split("x")[2].split("s")[0])
    assert kp % 16 == 0 and 8 * B <= kp < B * T, packed
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
def test_short_sequences_take_the_ungrouped_launches(gpu):
    B, T = 64, 8
    ih, _ = _full_dw_plans(B, T)
    assert "|gemm_p32_kernel<TN>" in ih and _splits(ih) > 1, ih     # only T < 16 keeps the group away
    kernels = _last_vs_full(1024, B, T)
    assert not _group_records(kernels), kernels
    assert any(k.startswith("gemm_p32_kernel<TN> %dx1024x%d " % (6 * H, B * T)) for k in kernels), kernels
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
def test_padded_input_width(gpu):
    """in = 1023: x, W_ih and dW_ih run at the padded width 1024 (the dwpad path, unpad_cols after the launch).  The
    full dW_ih plan there is still the split ping-pong kernel, so the group must engage; were it not, the fallback."""
    B, T = 24, 17
    ih, _ = _full_dw_plans(B, T, ld=1024)
    kernels = _last_vs_full(1023, B, T)
    if "|gemm_p32_kernel<TN>" in ih and _splits(ih) > 1:
        assert len(_group_records(kernels)) == 1, kernels
    else:
        assert not _group_records(kernels), kernels
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
def test_accumulates_into_prefilled_flat_gradients(gpu):
    """Gradients owned by FlatParams and pre-filled, two backward passes without zero_grad (beta = 1 in every GEMM
    epilogue and row-sum reduction): bitwise what the full layer leaves in the same buffers."""
    B, T = 24, 17
    sd, x, g = W.inputs(1024, B, T)
    fill = torch.randn(sum(v.numel() for v in sd.values()) + 4096, generator=torch.Generator().manual_seed(5))

    def two_passes(last):
        gru = W.device_gru(1024, sd)
        flat = FlatParams(gru.parameters())
        flat.grad.copy_(fill[:flat.grad.numel()].cuda())
        xg = x.cuda().requires_grad_(True)
        for _ in range(2):
            y = gru.forward_last(xg) if last else snn.last_step(gru(xg)[0])
            (y * g.cuda()).sum().backward()
        torch.cuda.synchronize()
        assert all(flat.owns_grad(p) for p in gru.parameters())
        return {"grad": flat.grad.clone(), "dx": xg.grad.clone()}

    full = two_passes(False)
    last, kernels = _profiled(lambda: two_passes(True))
    assert sum(k.startswith(W.GROUP_RECORD) for k in kernels) == 1, kernels   # one record, two launches
    _assert_equal(last, full)
    assert not torch.equal(last["grad"], fill[:last["grad"].numel()].cuda())
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
def test_graph_replays_equal_eager_step(gpu):
    """forward + backward + Adam at (24, 17) captured with GraphedStep: two replays from the same state are bitwise
    equal to each other and to the eager step from that state (whose launches include the group)."""
    B, T = 24, 17
    sd, x, g = W.inputs(1024, B, T, seed=13)
    gru = W.device_gru(1024, sd)
    flat = FlatParams(gru.parameters())
    opt = Adam(gru.parameters(), lr=1e-3, flat=flat)
    xs, gs = x.cuda(), g.cuda()

    def body():
        opt.zero_grad()
        loss = (gru.forward_last(xs) * gs).sum()
        loss.backward()
        opt.step()
        return loss

    opt.sync_lr()
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
    eager, kernels = _profiled(lambda: from_start(body))
    assert len(_group_records(kernels)) == 1, kernels
    for a, b, c in zip(r1, r2, eager):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(r1[1], start[0])   # the step moved the parameters
    assert _lib.spin_timeouts() == 0


@pytest.mark.gpu
def test_switch_off_in_a_child_process_gives_the_same_bits(gpu, tmp_path):
    """SRK_GEMM_GROUP=0 (read once per process) turns the group off: a child process computes the (24, 17) case with
    the ungrouped launches, and its results equal the grouped ones of this process bit for bit."""
    B, T = 24, 17
    out = str(tmp_path / "ungrouped.pt")
    env = dict(os.environ, SRK_GEMM_GROUP="0")
    r = subprocess.run([sys.executable, os.path.join(W.HERE, "bigru_group_worker.py"), "1024", str(B), str(T), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = torch.load(out)
    sd, x, g = W.inputs(1024, B, T)
    last, kernels = _profiled(lambda: W.run(W.device_gru(1024, sd), x, g, True))
    assert len(_group_records(kernels)) == 1, kernels
    _assert_equal({k: v.cpu() for k, v in last.items()}, child)
    assert _lib.spin_timeouts() == 0
