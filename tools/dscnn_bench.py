"""Depthwise-conv / DS-CNN benchmark: writes profiles/dscnn_bench.json.

    python tools/dscnn_bench.py [--rounds 7] [--iters 20] [--batch 512]

One process, alternating rounds, fp32 channels-last tensors, the four depthwise layers of fbanks_dscnn at batch 512
(ds1 98x40x64 stride (1,2), ds2 98x20x128 stride (1,1), ds3 98x20x128 stride (2,2), ds4 49x10x256 stride (1,1); all
3 x 3, padding 1):

(a) srk_dwconv2d_nhwc_fwd, srk_dwconv2d_nhwc_bwd whole ("bwd") and with dx = NULL ("wgrad": both of its launches), the
    data gradient alone from the library's per-launch event timers (it has no entry point of its own), and
    srk_avgpool_nhwc_fwd / _bwd on the plugin's [512, 490, 256], with the achieved GB/s over the ALGORITHMIC bytes,
    nx = N H W C and ny = N Ho Wo C floats:
        fwd    4 (nx + ny + 9 C)            x read once, y written once, the weights
        dgrad  4 (ny + nx + 9 C)            dY read once, dx written once
        wgrad  4 (nx + ny + 10 C)           x and dY read once, dw and db written (the slabs are not algorithmic)
        avgpool fwd / bwd  4 (N HW C + N C)
(b) next to each: torch.nn.functional.conv2d(groups=C) on channels-last (memory_format) tensors, forward and
    autograd backward (both gradients in one call), and a plain ``copy_`` of the SAME byte count (a float32 buffer
    of bytes / 2 elements copied: bytes / 2 read + bytes / 2 written) measured in the same rounds — the yardstick
    for "memory-bound";
(c) the fbanks_dscnn train step (forward, loss, backward, Adam) replayed from a HIP graph next to fbanks_cnn's at
    the same batch, in fp32 and bf16: ms per step and utt/s, with the eager step's per-category kernel times.

Each round times every variant once (--iters calls between two device events); the figure is the median over rounds,
the spread the (max - min) / median of the rounds.  Times are device-event times of whole calls.  The tensors of one
layer (up to 0.5 GB each) do not fit the 256 MB last-level cache together, so the figures are HBM figures.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from speechrecognitionproject_amd import _lib, nn as snn  # noqa: E402
from speechrecognitionproject_amd.features import ptr, stream_ptr  # noqa: E402

LAYERS = {"ds1": (98, 40, 64, 1, 2), "ds2": (98, 20, 128, 1, 1), "ds3": (98, 20, 128, 2, 2), "ds4": (49, 10, 256, 1, 1)}


def time_calls(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters   # ms per call


def summarize(samples):
    med = statistics.median(samples)
    return {"us": round(med * 1e3, 2), "spread": round((max(samples) - min(samples)) / med, 4), "rounds": len(samples)}


def run_variants(variants, rounds):
    """variants: name -> (call, algorithmic bytes or None, iterations); alternating rounds."""
    for call, _, _ in variants.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (call, _, it) in variants.items():
            samples[v].append(time_calls(call, it))
    res = {}
    for v, (_, nbytes, _) in variants.items():
        e = summarize(samples[v])
        if nbytes:
            e["bytes"] = nbytes
            e["gb_per_s"] = round(nbytes / (e["us"] * 1e-6) / 1e9, 1)
        res[v] = e
    return res


def copy_call(nbytes):
    n = int(nbytes // 8)
    src = torch.empty(n, device="cuda").normal_()
    dst = torch.empty(n, device="cuda")
    return lambda: dst.copy_(src)


def bench_layer(N, H, W, C, sh, sw, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    Ho, Wo = (H + 2 - 3) // sh + 1, (W + 2 - 3) // sw + 1
    x = torch.randn(N, H, W, C, device="cuda", generator=g)
    w = torch.randn(C, 1, 3, 3, device="cuda", generator=g) / 3
    dy = torch.randn(N, Ho, Wo, C, device="cuda", generator=g)
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
    geom = (N, H, W, C, 3, 3, 1, 1, sh, sw)
    ws = torch.empty(int(_lib.lib().srk_dwconv2d_workspace_floats(*geom)), device="cuda")

    def fwd():
        _lib.call("srk_dwconv2d_nhwc_fwd", ptr(x), N, H, W, C, ptr(w), None, 3, 3, 1, 1, sh, sw, ptr(y), stream_ptr())

    def bwd(dxo):
        return lambda: _lib.call("srk_dwconv2d_nhwc_bwd", ptr(x), N, H, W, C, ptr(w), 3, 3, 1, 1, sh, sw, ptr(dy), dxo,
                                 ptr(dw), None, ptr(ws), 0, stream_ptr())

    # torch: NCHW-shaped views of the same channels-last memory
    xt = x.permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.clone().requires_grad_(True)
    dyt = dy.permute(0, 3, 1, 2)
    state = {}

    def torch_fwd():
        state["y"] = F.conv2d(xt, wt, None, stride=(sh, sw), padding=1, groups=C)

    def torch_bwd():
        torch.autograd.grad(state["y"], (xt, wt), dyt, retain_graph=True)

    nx, ny = float(N) * H * W * C, float(N) * Ho * Wo * C
    b_fwd, b_wgrad = 4.0 * (nx + ny + 9 * C), 4.0 * (nx + ny + 10 * C)
    variants = {
        "fwd": (fwd, b_fwd, iters),
        "bwd": (bwd(ptr(dx)), b_fwd + b_wgrad, iters),
        "wgrad": (bwd(None), b_wgrad, iters),
        "copy_fwd_bytes": (copy_call(b_fwd), b_fwd, iters),
        "copy_bwd_bytes": (copy_call(b_fwd + b_wgrad), b_fwd + b_wgrad, iters),
        "torch_fwd": (torch_fwd, b_fwd, max(2, iters // 4)),
        "torch_bwd": (torch_bwd, b_fwd + b_wgrad, max(2, iters // 4)),
    }
    res = run_variants(variants, rounds)
    fwd()
    torch_fwd()
    torch.cuda.synchronize()
    ref = state["y"].detach().permute(0, 2, 3, 1)
    res["fwd_vs_torch_rel_err"] = float((y - ref).abs().max() / ref.abs().max())
    # the data gradient has no entry point of its own: the library's per-launch event timers split the backward call
    try:
        _lib.prof_enable(1)
        for _ in range(rounds):
            bwd(ptr(dx))()
        torch.cuda.synchronize()
        n, ms, _ = _lib.prof_read("dwconv_dgrad")
        n2, ms2, _ = _lib.prof_read("dwconv_wgrad")
    finally:
        _lib.prof_enable(0)
    dg = {"us": round(ms / n * 1e3, 2), "bytes": b_fwd, "launches_timed": n, "timer": "per-launch events (mean)"}
    dg["gb_per_s"] = round(b_fwd / (dg["us"] * 1e-6) / 1e9, 1)
    res["dgrad"] = dg
    res["wgrad_launch_pair_us_by_launch_timers"] = round(ms2 / (n2 / 2) * 1e3, 2)
    copy = res["copy_fwd_bytes"]["gb_per_s"]
    res["fwd_over_copy_bw"] = round(res["fwd"]["gb_per_s"] / copy, 3)
    res["dgrad_over_copy_bw"] = round(dg["gb_per_s"] / copy, 3)
    res["wgrad_over_copy_bw"] = round(res["wgrad"]["gb_per_s"] / copy, 3)
    res["shape"] = {"N": N, "H": H, "W": W, "C": C, "stride": [sh, sw], "Ho": Ho, "Wo": Wo}
    return res


def bench_avgpool(N, HW, C, rounds, iters):
    x = torch.randn(N, HW, C, device="cuda")
    dy = torch.randn(N, C, device="cuda")
    y, dx = torch.empty(N, C, device="cuda"), torch.empty_like(x)
    nbytes = 4.0 * (float(N) * HW * C + N * C)
    variants = {
        "fwd": (lambda: _lib.call("srk_avgpool_nhwc_fwd", ptr(x), N, HW, C, ptr(y), stream_ptr()), nbytes, iters),
        "bwd": (lambda: _lib.call("srk_avgpool_nhwc_bwd", ptr(dy), N, HW, C, ptr(dx), stream_ptr()), nbytes, iters),
        "copy_same_bytes": (copy_call(nbytes), nbytes, iters),
        "torch_mean": (lambda: x.mean(dim=1), nbytes, iters),
    }
    res = run_variants(variants, rounds)
    res["shape"] = [N, HW, C]
    return res


def make_step(model, N):
    from speechrecognitionproject_amd.optim import Adam, FlatParams
    from speechrecognitionproject_amd.synthetic import synthetic_clips
    torch.manual_seed(0)
    net = importlib.import_module("speechrecognitionproject_amd.models.model_" + model).Network().cuda()
    net.train()
    flat = FlatParams(net.parameters())
    opt = Adam(net.parameters(), lr=1e-4, flat=flat)
    crit = snn.CrossEntropyLoss()
    x, y = synthetic_clips(N, seed=3)
    sx, sy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()

    def body():
        opt.zero_grad()
        loss = crit(net(sx), sy)
        loss.backward()
        opt.step()
        return loss

    return body


def eager_kernel_times(body):
    """{category: ms} of one eager step (the library's per-launch event timers; graphs are timed without them)."""
    for _ in range(2):
        body()
    try:
        _lib.prof_enable(1)
        body()
        torch.cuda.synchronize()
        by = {}
        for k in _lib.prof_kernels():
            by[k["name"]] = by.get(k["name"], 0.0) + k["ms_total"]
    finally:
        _lib.prof_enable(0)
    return {k: round(v, 4) for k, v in sorted(by.items(), key=lambda kv: -kv[1])}


def bench_steps(N, prec, rounds, replays):
    """fbanks_dscnn and fbanks_cnn steps at one precision, their graphs replayed in alternating rounds."""
    from speechrecognitionproject_amd.graphs import GraphedStep
    _lib.set_matmul_precision(prec)
    try:
        res, graphs, bodies = {}, {}, {}
        # every eager pass first: the library's grow-only scratch buffers reach both models' sizes before a capture
        for m in ("fbanks_dscnn", "fbanks_cnn"):
            bodies[m] = make_step(m, N)
            res[m] = {"eager_kernel_ms": eager_kernel_times(bodies[m])}
        for m, body in bodies.items():
            graphs[m] = GraphedStep(body, warmup=2)
            for _ in range(3):
                graphs[m].replay()
        torch.cuda.synchronize()
        samples = {m: [] for m in graphs}
        for _ in range(rounds):
            for m, g in graphs.items():
                samples[m].append(time_calls(g.replay, replays))
        for m, g in graphs.items():
            loss = float(g.replay().item())
            e = summarize(samples[m])
            e["ms"] = round(e.pop("us") * 1e-3, 5)
            e["utt_per_s"] = round(N / (e["ms"] * 1e-3), 1)
            e["loss_finite"] = bool(loss == loss and abs(loss) != float("inf"))
            res[m].update(e)
            g.release()
        res["dscnn_over_cnn_ms"] = round(res["fbanks_dscnn"]["ms"] / res["fbanks_cnn"]["ms"], 4)
        return res
    finally:
        _lib.set_matmul_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dscnn_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (c), the graphed train steps")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dscnn_bench needs a GPU: no timing without one")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "batch": a.batch,
           "source_stamp": _lib.source_stamp(), "kernels": {}, "train_step_graph": {"batch": a.batch}}
    for name, (H, W, C, sh, sw) in LAYERS.items():
        out["kernels"][name] = bench_layer(a.batch, H, W, C, sh, sw, a.rounds, a.iters)
        torch.cuda.empty_cache()
    out["avgpool"] = bench_avgpool(a.batch, 490, 256, a.rounds, a.iters)
    torch.cuda.empty_cache()
    if not a.no_step:
        for prec in ("fp32", "bf16"):
            out["train_step_graph"][prec] = bench_steps(a.batch, prec, a.rounds, max(2, a.iters // 4))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
