"""PCEN benchmark: writes profiles/pcen_bench.json.

    python tools/pcen_bench.py [--rounds 7] [--iters 50]

One process, alternating rounds, the plugin's shape T = 98, C = 120 at B = 256 and B = 512 (fp32 tensors):

(a) srk_pcen_fwd (training form: y and M written) and srk_pcen_bwd (the plugin's form: dx = NULL; both of its
    launches) with the achieved GB/s over the ALGORITHMIC bytes (fwd: x read, y and M written; bwd: x, M, dy read,
    the columns' parameter sums written and read), and the evaluation forward (no M) and the backward with dx, next
    to
(b) the same arithmetic as a 98-step loop of torch device ops on the same tensors ("torch"; its backward is
    autograd's), for scale, and
(c) the fbanks_cnn_pcen train step (forward, loss, backward, Adam) replayed from a HIP graph next to fbanks_cnn's at
    batch 512, in fp32 and bf16: ms per step and utt/s, with the eager step's per-category kernel times of both
    models from the library's profiler (where the difference goes).

Each round times every variant once (--iters calls between two device events); the figure is the median over
rounds, the spread the (max - min) / median of the rounds.  Times are device-event times of whole calls.
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from speechrecognitionproject_amd import _lib, nn as snn  # noqa: E402
from speechrecognitionproject_amd.features import ptr, stream_ptr  # noqa: E402

K_DB, EPS = math.log(10.0) / 20.0, 1e-6


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


def torch_pcen(x, p):
    alpha, delta, r, s = p[0].exp(), p[1].exp(), p[2].exp(), torch.sigmoid(p[3])
    E = torch.exp(K_DB * x)
    Ms = [E[:, 0]]
    for t in range(1, x.shape[1]):
        Ms.append((1 - s) * Ms[-1] + s * E[:, t])
    M = torch.stack(Ms, dim=1)
    return (E * (EPS + M) ** (-alpha) + delta) ** r - delta ** r


def bench_kernels(B, T, C, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 20.0 + 200.0 * torch.rand(B, T, C, device="cuda", generator=g)
    p = snn.PCEN(C).params.detach().cuda() + 0.1 * torch.randn(4, C, device="cuda", generator=g)
    dy = torch.randn(B, T, C, device="cuda", generator=g)
    y, m, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    dp = torch.empty_like(p)
    ws = torch.empty(int(_lib.lib().srk_pcen_workspace_floats(B, T, C)), device="cuda")

    def fwd(mo):
        return lambda: _lib.call("srk_pcen_fwd", ptr(x), ptr(p), B, T, C, K_DB, EPS, ptr(y), mo, stream_ptr())

    def bwd(dxo):
        return lambda: _lib.call("srk_pcen_bwd", ptr(x), ptr(p), ptr(m), ptr(dy), B, T, C, K_DB, EPS, dxo, ptr(dp),
                                 ptr(ws), stream_ptr())

    pt = p.clone().requires_grad_(True)
    state = {}

    def torch_fwd():
        state["y"] = torch_pcen(x, pt)

    def torch_bwd():
        torch.autograd.grad(state["y"], pt, dy, retain_graph=True)

    n = float(B) * T * C
    variants = {   # name -> (call, algorithmic bytes, iterations)
        "fwd": (fwd(ptr(m)), 4.0 * (3 * n + 4 * C), iters),
        "fwd_eval": (fwd(None), 4.0 * (2 * n + 4 * C), iters),
        "bwd": (bwd(None), 4.0 * (3 * n + 12 * C + 8 * B * C), iters),
        "bwd_dx": (bwd(ptr(dx)), 4.0 * (4 * n + 12 * C + 8 * B * C), iters),
        "torch_fwd": (torch_fwd, 4.0 * (3 * n + 4 * C), max(2, iters // 10)),
        "torch_bwd": (torch_bwd, 4.0 * (3 * n + 12 * C + 8 * B * C), max(2, iters // 10)),
    }
    for call, _, _ in variants.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    variants["fwd"][0]()
    torch.cuda.synchronize()
    agree = float((y - state["y"].detach()).abs().max() / state["y"].detach().abs().max())
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (call, _, it) in variants.items():
            samples[v].append(time_calls(call, it))
    res = {"shape": [B, T, C], "fused_vs_torch_y_rel_err": agree}
    for v, (_, nbytes, _) in variants.items():
        e = summarize(samples[v])
        e["bytes"] = nbytes
        e["gb_per_s"] = round(nbytes / (e["us"] * 1e-6) / 1e9, 1)   # algorithmic bytes, also for torch
        res[v] = e
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
    """fbanks_cnn_pcen and fbanks_cnn steps at one precision, their graphs replayed in alternating rounds."""
    from speechrecognitionproject_amd.graphs import GraphedStep
    _lib.set_matmul_precision(prec)
    try:
        res, graphs = {}, {}
        for m in ("fbanks_cnn_pcen", "fbanks_cnn"):
            body = make_step(m, N)
            res[m] = {"eager_kernel_ms": eager_kernel_times(body)}
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
        res["pcen_over_plain_ms"] = round(res["fbanks_cnn_pcen"]["ms"] / res["fbanks_cnn"]["ms"], 4)
        return res
    finally:
        _lib.set_matmul_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcen_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (c), the graphed train steps")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcen_bench needs a GPU: no timing without one")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters,
           "source_stamp": _lib.source_stamp(),
           "kernels": {str(B): bench_kernels(B, 98, 120, a.rounds, a.iters) for B in (256, 512)},
           "train_step_graph": {"batch": a.step_batch}}
    if not a.no_step:
        for prec in ("fp32", "bf16"):
            out["train_step_graph"][prec] = bench_steps(a.step_batch, prec, a.rounds, max(2, a.iters // 5))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
