"""Attention-pooling benchmark: writes profiles/attn_bench.json.

    python tools/attn_bench.py [--batch 256] [--rounds 7] [--iters 50]

One process, alternating rounds, the model shape B = 256, T = 51, D = 1024 (fp32 tensors):

(a) the pool's forward and backward through srk_attn_pool_fwd / _bwd — the register-resident kernel the shape takes
    by default ("fused") and the two-pass kernel every other shape takes ("fused_2pass", attn_pool_regs = 0) — with
    the achieved GB/s over the ALGORITHMIC bytes (fwd: y read once + q, ctx, alpha; bwd: y read and dy written once
    + q, dctx, dq, alpha), next to
(b) the same pool built from torch device ops on the same tensors ("torch": bmm, softmax, bmm; its backward is
    autograd's), which is the yardstick, and
(c) the mfcc_bgru_att train step (forward, loss, backward, Adam) replayed from a HIP graph next to mfcc_bgru's at
    the same batch, in fp32 and bf16: ms per step and utt/s.

Each round times every variant once (--iters calls between two device events); the figure is the median over
rounds, the spread the (max - min) / median of the rounds.  Times are device-event times of whole calls.
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

from speechrecognitionproject_amd import _lib, nn as snn  # noqa: E402
from speechrecognitionproject_amd.features import ptr, stream_ptr  # noqa: E402


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
    return {"ms": round(med, 5), "spread": round((max(samples) - min(samples)) / med, 4), "rounds": len(samples)}


def pool_variants(B, T, D):
    """{variant: (fwd(), bwd())} closures over the same preallocated tensors."""
    g = torch.Generator(device="cuda").manual_seed(1)
    y = torch.rand(B, T, D, device="cuda", generator=g) * 2 - 1
    q = torch.randn(B, D, device="cuda", generator=g)
    dctx = torch.randn(B, D, device="cuda", generator=g)
    scale = D ** -0.5
    ctx, alpha = torch.empty(B, D, device="cuda"), torch.empty(B, T, device="cuda")
    dy, dq = torch.empty_like(y), torch.empty_like(q)

    def fused():
        def fwd():
            _lib.call("srk_attn_pool_fwd", ptr(y), ptr(q), B, T, D, scale, ptr(ctx), ptr(alpha), stream_ptr())

        def bwd():
            _lib.call("srk_attn_pool_bwd", ptr(y), ptr(q), ptr(alpha), ptr(dctx), B, T, D, scale, ptr(dy), ptr(dq),
                      stream_ptr())
        return fwd, bwd

    yt, qt = y.clone().requires_grad_(True), q.clone().requires_grad_(True)
    state = {}

    def torch_fwd():
        a = torch.softmax(torch.bmm(yt, qt.unsqueeze(2)).squeeze(2) * scale, dim=1)
        state["ctx"] = torch.bmm(a.unsqueeze(1), yt).squeeze(1)

    def torch_bwd():   # the backward of the last torch_fwd's graph
        torch.autograd.grad(state["ctx"], (yt, qt), dctx, retain_graph=True)

    return {"fused": fused(), "fused_2pass": fused(), "torch": (torch_fwd, torch_bwd)}, (ctx, dy, dq, state)


def bench_pool(B, T, D, rounds, iters):
    variants, keep = pool_variants(B, T, D)
    regs = lambda v: _lib.options(attn_pool_regs=0 if v == "fused_2pass" else 1)   # noqa: E731
    for v, (fwd, bwd) in variants.items():
        with regs(v):
            for _ in range(3):
                fwd()
                bwd()
    torch.cuda.synchronize()
    # the fused forward against the torch-composed one, on the timed tensors
    with regs("fused"):
        variants["fused"][0]()
    variants["torch"][0]()
    torch.cuda.synchronize()
    ref = keep[3]["ctx"].detach()
    agree = float((keep[0] - ref).abs().max() / ref.abs().max())
    samples = {(v, d): [] for v in variants for d in ("fwd", "bwd")}
    for _ in range(rounds):
        for v, (fwd, bwd) in variants.items():
            with regs(v):   # (between timed windows)
                samples[v, "fwd"].append(time_calls(fwd, iters))
                samples[v, "bwd"].append(time_calls(bwd, iters))
    nbytes = {"fwd": 4.0 * (B * T * D + 2 * B * D + B * T), "bwd": 4.0 * (2 * B * T * D + 3 * B * D + B * T)}
    res = {"shape": [B, T, D], "bytes_fwd": nbytes["fwd"], "bytes_bwd": nbytes["bwd"],
           "fused_vs_torch_ctx_rel_err": agree}
    for (v, d), s in samples.items():
        e = summarize(s)
        e["gb_per_s"] = round(nbytes[d] / (e["ms"] * 1e-3) / 1e9, 1)   # algorithmic bytes, also for torch
        res["%s_%s" % (v, d)] = e
    for d in ("fwd", "bwd"):
        res["speedup_%s_vs_torch" % d] = round(res["torch_" + d]["ms"] / res["fused_" + d]["ms"], 3)
    return res


def graphed_step(model, N, prec):
    from speechrecognitionproject_amd.graphs import GraphedStep
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

    g = GraphedStep(body, warmup=2)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def bench_steps(N, prec, rounds, replays):
    """mfcc_bgru_att and mfcc_bgru steps at one precision, their graphs replayed in alternating rounds."""
    _lib.set_matmul_precision(prec)
    try:
        graphs = {m: graphed_step(m, N, prec) for m in ("mfcc_bgru_att", "mfcc_bgru")}
        samples = {m: [] for m in graphs}
        for _ in range(rounds):
            for m, g in graphs.items():
                samples[m].append(time_calls(g.replay, replays))
        res = {}
        for m, g in graphs.items():
            loss = float(g.replay().item())
            e = summarize(samples[m])
            e["utt_per_s"] = round(N / (e["ms"] * 1e-3), 1)
            e["loss_finite"] = bool(loss == loss and abs(loss) != float("inf"))
            res[m] = e
            g.release()
        res["att_over_plain_ms"] = round(res["mfcc_bgru_att"]["ms"] / res["mfcc_bgru"]["ms"], 4)
        return res
    finally:
        _lib.set_matmul_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (c), the graphed train steps")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench needs a GPU: no timing without one")
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "rounds": a.rounds, "iters": a.iters,
           "source_stamp": _lib.source_stamp(), "pool": bench_pool(a.batch, 51, 1024, a.rounds, a.iters),
           "train_step_graph": {}}
    if not a.no_step:
        for prec in ("fp32", "bf16"):
            out["train_step_graph"][prec] = bench_steps(a.batch, prec, a.rounds, max(2, a.iters // 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
