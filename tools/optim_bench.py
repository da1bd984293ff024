"""Optimizer-extension benchmark (AdamW decay, global-norm clipping, weight EMA): writes profiles/optim_bench.json.

    python tools/optim_bench.py [--rounds 7] [--iters 50]

One process, alternating rounds:

(a) at the flat parameter counts of mfcc_bgru and fbanks_cnn: the gradient-norm pass (srk_adamw_step's first launch,
    4 B n read) next to a device copy (torch ``copy_``, 8 B n) of the same buffer, and the update loop with decay, clip
    and EMA all on (adam_state_kernel, 28 B n + 8 B n + n / 64 B, key "adamw_kernel") next to the same loop with
    everything off (adam_plain_kernel, 28 B n; the key is still "adam_state_kernel") on the same buffers.  The
    kernels alone come from the library's event pair around each launch (srk_prof categories "grad_norm", "adamw", "adam"), one mean per
    round; the whole calls (prep launch and host cost included) from device events around --iters calls.  The finite
    check of a loss-scaled step (grad_norm_kernel<false>, category "grad_check", 4 B n) is timed the same way through
    srk_adam_step_scaled ("grad_check_kernel") and through srk_adamw_step with a scaler alone
    ("grad_check_adamw_kernel");
(b) the mfcc_bgru (cfg2: batch 256, fp32) and fbanks_cnn train steps (forward, loss, backward, optimizer) replayed
    from a HIP graph, without the flags and with ``--clip-grad-norm 1 --weight-decay 0.01 --ema 0.999`` in the same
    rounds: ms per step, utt/s and the ratio, beside the spread of the same run, and next to it what the extra bytes
    (4 B n + 8 B n + n / 64 B) cost at the copy's bandwidth.

Each round times every variant once; the figure is the median over rounds, the spread the (max - min) / median of
the rounds.  Buffers of these sizes fit the 256 MiB Infinity Cache when called back to back, so the GB/s of (a) are
cache-resident rates, not HBM rates.
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
from speechrecognitionproject_amd.optim import Adam, FlatParams  # noqa: E402

STEP_MODELS = ("mfcc_bgru", "fbanks_cnn")
MAX_NORM, WD, EMA = 1.0, 0.01, 0.999
B1, B2, EPS = 0.9, 0.999, 1e-8


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


def flat_numel(model):
    """The flat parameter count of a plugin (every tensor padded to 64 floats), without touching the GPU."""
    from speechrecognitionproject_amd.optim import flat_layout
    net = importlib.import_module("speechrecognitionproject_amd.models.model_" + model).Network()
    return flat_layout(net.parameters())[2]


def bench_kernels(n, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(n, device="cuda", generator=g)
    grad = torch.randn(n, device="cuda", generator=g)
    m, v, ema, dst = torch.zeros_like(p), torch.zeros_like(p), p.clone(), torch.empty_like(p)
    mask = (torch.arange((n + 63) // 64, device="cuda") % 4 != 3).to(torch.uint8)
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    st.view(torch.float32)[4] = 1e-4
    clip = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(_lib.lib().srk_adamw_workspace_floats(n)), device="cuda")

    def old():
        _lib.call("srk_adam_step_state", ptr(p), ptr(grad), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), 1.0, stream_ptr())

    def new():
        _lib.call("srk_adamw_step", ptr(p), ptr(grad), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), 1.0, None, WD,
                  ptr(mask), MAX_NORM, ptr(clip), ptr(ema), EMA, ptr(ws), stream_ptr())

    variants = {"copy": (lambda: dst.copy_(grad), 8.0 * n), "adam_step_state_call": (old, None),
                "adamw_step_call": (new, None)}
    for call, _ in variants.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (call, _) in variants.items():
            samples[k].append(time_calls(call, iters))
    res = {"n": n}
    for k, (_, nbytes) in variants.items():
        e = summarize(samples[k])
        if nbytes is not None:
            e["bytes"] = nbytes
            e["gb_per_s"] = round(nbytes / (e["us"] * 1e-6) / 1e9, 1)
        res[k] = e
    # the kernels alone, by the library's own event pair around each launch
    cats = (("grad_norm", "norm_kernel"), ("adamw", "adamw_kernel"), ("adam", "adam_state_kernel"))
    per_round, per_launch_bytes = {key: [] for _, key in cats}, {}
    for _ in range(rounds):
        _lib.prof_enable(True)
        for _ in range(iters):
            old()
            new()
        torch.cuda.synchronize()
        for name, key in cats:
            launches, ms, nbytes = _lib.prof_read(name)
            per_round[key].append(ms / launches)
            per_launch_bytes[key] = nbytes / launches
        _lib.prof_enable(False)
    for _, key in cats:
        e = summarize(per_round[key])
        e.update(launches=rounds * iters, bytes=per_launch_bytes[key],
                 gb_per_s=round(per_launch_bytes[key] / (e["us"] * 1e-6) / 1e9, 1))
        res[key] = e
    # the finite check of a scaled step (static scale, finite gradients: every step updates), through both entries
    sc = torch.zeros(8, dtype=torch.int32, device="cuda")
    _lib.call("srk_grad_scaler_init", ptr(sc), 1.0, 2.0, 0.5, 0, stream_ptr())
    checks = {"grad_check_kernel": lambda: _lib.call(
                  "srk_adam_step_scaled", ptr(p), ptr(grad), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), 1.0, ptr(sc),
                  stream_ptr()),
              "grad_check_adamw_kernel": lambda: _lib.call(
                  "srk_adamw_step", ptr(p), ptr(grad), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), 1.0, ptr(sc), 0.0, None,
                  0.0, None, None, 0.0, None, stream_ptr())}
    per_round = {k: [] for k in checks}
    for _ in range(rounds):
        for key, call in checks.items():
            _lib.prof_enable(True)
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            launches, ms, nbytes = _lib.prof_read("grad_check")
            _lib.prof_enable(False)
            per_round[key].append(ms / launches)
    for key, samples in per_round.items():
        res[key] = dict(summarize(samples), bytes=4.0 * n)
    res["norm_over_copy"] = round(res["norm_kernel"]["us"] / res["copy"]["us"], 3)
    res["adamw_over_adam_kernel"] = round(res["adamw_kernel"]["us"] / res["adam_state_kernel"]["us"], 3)
    res["adamw_over_adam_bytes"] = round(res["adamw_kernel"]["bytes"] / res["adam_state_kernel"]["bytes"], 3)
    res["clip_state"] = {"total_norm": clip.view(torch.float32)[0].item(), "coef": clip.view(torch.float32)[1].item(),
                         "clipped_steps": clip[2].item()}
    return res


def make_step(model, N, extended):
    """training.py's eager_step on a resident batch, with or without the three optimizer flags."""
    from speechrecognitionproject_amd.synthetic import synthetic_clips
    torch.manual_seed(0)
    net = importlib.import_module("speechrecognitionproject_amd.models.model_" + model).Network().cuda()
    net.train()
    flat = FlatParams(net.parameters())
    kw = dict(weight_decay=WD, max_grad_norm=MAX_NORM, ema_decay=EMA) if extended else {}
    opt = Adam(net.parameters(), lr=1e-4, flat=flat, **kw)
    crit = snn.CrossEntropyLoss()
    x, y = synthetic_clips(N, seed=3)
    sx, sy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()

    def body():
        opt.zero_grad()
        loss = crit(net(sx), sy)
        loss.backward()
        opt.step()
        return loss

    return body, opt


def bench_steps(model, N, rounds, replays, copy_gb_per_s):
    from speechrecognitionproject_amd.graphs import GraphedStep
    steps = {"plain": make_step(model, N, False), "extended": make_step(model, N, True)}
    graphs = {k: GraphedStep(body, warmup=2) for k, (body, _) in steps.items()}
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    samples = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            samples[k].append(time_calls(g.replay, replays))
    opt = steps["extended"][1]
    n = opt.flat.numel
    res = {"flat_numel": n, "max_grad_norm": MAX_NORM, "weight_decay": WD, "ema_decay": EMA}
    for k, g in graphs.items():
        loss = float(g.replay().item())
        e = summarize(samples[k])
        e["ms"] = round(e.pop("us") * 1e-3, 5)
        e["utt_per_s"] = round(N / (e["ms"] * 1e-3), 1)
        e["loss_finite"] = bool(loss == loss and abs(loss) != float("inf"))
        res[k] = e
        g.release()
    res["extended"]["clipped_steps"] = opt.clipped_steps()
    res["extended"]["last_grad_norm"] = opt.last_grad_norm()
    res["extended_over_plain_ms"] = round(res["extended"]["ms"] / res["plain"]["ms"], 4)
    extra_bytes = (4.0 + 8.0 + 1.0 / 64.0) * n
    res["extra_bytes"] = extra_bytes
    res["extra_ms_measured"] = round(res["extended"]["ms"] - res["plain"]["ms"], 5)
    res["extra_ms_at_copy_bandwidth"] = round(extra_bytes / (copy_gb_per_s * 1e9) * 1e3, 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256, help="batch of the graphed train steps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (b), the graphed train steps")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a GPU: no timing without one")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters,
           "source_stamp": _lib.source_stamp(), "kernels": {}, "train_step_graph": {"batch": a.batch}}
    for model in STEP_MODELS:
        out["kernels"][model] = bench_kernels(flat_numel(model), a.rounds, a.iters)
    if not a.no_step:
        for model in STEP_MODELS:
            out["train_step_graph"][model] = bench_steps(model, a.batch, a.rounds, max(2, a.iters // 5),
                                                         out["kernels"][model]["copy"]["gb_per_s"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
