"""SpecAugment benchmark: writes profiles/specaug_bench.json.

    python tools/specaug_bench.py [--rounds 7] [--iters 50]

One process, alternating rounds, 512 clips of each of the three model feature shapes (MFCC 51 x 39, filter banks
98 x 120, spectrogram 49 x 321; time-major fp32, the tensors the plugins feed their networks):

(a) srk_specaug_apply with drawn parameters of the shape's policy, out of place and in place, mean and zero fill,
    and on the freq-major transpose, next to a device copy (torch ``copy_``) of the same tensor — the kernel reads
    and writes each element once, as the copy does — with the achieved GB/s over the algorithmic bytes;
(b) the draw launch (srk_specaug_draw) for the 512 clips;
(c) the mfcc_bgru and fbanks_cnn train steps (forward, loss, backward, Adam) replayed from a HIP graph at batch
    512, fp32 and bf16, with and without ``specaug=`` in the same rounds: ms per step, utt/s and the ratio.

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

from speechrecognitionproject_amd import _lib, features as K, nn as snn  # noqa: E402

SHAPES = {"mfcc_51x39": ((51, 39), (3, 2, 6, 2, 8)), "fbank_98x120": ((98, 120), (5, 2, 15, 2, 12)),
          "spec_49x321": ((49, 321), (4, 2, 40, 2, 8))}
STEP_MODELS = {"mfcc_bgru": (5, 2, 15, 2, 12), "fbanks_cnn": (5, 2, 15, 2, 12)}    # --specaug 5,2,15,2,12 on both


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


def bench_kernels(B, T, F, policy, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 20.0 * torch.randn(B, T, F, device="cuda", generator=g)
    xt = x.transpose(1, 2).contiguous()
    y, yt, work = torch.empty_like(x), torch.empty_like(xt), x.clone()
    mean, zero = K.specaug_policy(*policy), K.specaug_policy(*policy, fill="zero")
    K.specaug_reseed(1234)
    params = K.specaug_draw(B, T, F, mean)
    buf = torch.empty_like(params)
    n = float(B) * T * F
    apply_bytes = 8.0 * n + 4.0 * params.numel()
    variants = {   # name -> (call, algorithmic bytes)
        "copy": (lambda: y.copy_(x), 8.0 * n),
        "apply_mean": (lambda: K.spec_augment(x, params, mean, out=y), apply_bytes),
        "apply_zero": (lambda: K.spec_augment(x, params, zero, out=y), apply_bytes),
        "apply_mean_in_place": (lambda: K.spec_augment(work, params, mean, out=work), apply_bytes),
        "apply_mean_freq_major": (lambda: K.spec_augment(xt, params, mean, time_major=False, out=yt), apply_bytes),
        "draw": (lambda: K.specaug_draw(B, T, F, mean, out=buf), 4.0 * params.numel()),
    }
    for call, _ in variants.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (call, _) in variants.items():
            samples[v].append(time_calls(call, iters))
    p = params.cpu()
    res = {"shape": [B, T, F], "policy": list(policy), "clips_warped": int((p[:, 0] != p[:, 1]).sum())}
    for v, (_, nbytes) in variants.items():
        e = summarize(samples[v])
        e["bytes"] = nbytes
        e["gb_per_s"] = round(nbytes / (e["us"] * 1e-6) / 1e9, 1)
        res[v] = e
    res["apply_mean_over_copy"] = round(res["apply_mean"]["us"] / res["copy"]["us"], 3)
    return res


def make_step(model, N, specaug):
    from speechrecognitionproject_amd.optim import Adam, FlatParams
    from speechrecognitionproject_amd.synthetic import synthetic_clips
    torch.manual_seed(0)
    net = importlib.import_module("speechrecognitionproject_amd.models.model_" + model).Network(specaug=specaug).cuda()
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


def bench_steps(model, N, prec, rounds, replays):
    """One model's step with and without SpecAugment at one precision, the two graphs replayed in alternating rounds."""
    from speechrecognitionproject_amd.graphs import GraphedStep
    _lib.set_matmul_precision(prec)
    try:
        graphs = {"plain": GraphedStep(make_step(model, N, None), warmup=2),
                  "specaug": GraphedStep(make_step(model, N, STEP_MODELS[model]), warmup=2)}
        for g in graphs.values():
            for _ in range(3):
                g.replay()
        torch.cuda.synchronize()
        samples = {m: [] for m in graphs}
        for _ in range(rounds):
            for m, g in graphs.items():
                samples[m].append(time_calls(g.replay, replays))
        res = {"policy": list(STEP_MODELS[model])}
        for m, g in graphs.items():
            loss = float(g.replay().item())
            e = summarize(samples[m])
            e["ms"] = round(e.pop("us") * 1e-3, 5)
            e["utt_per_s"] = round(N / (e["ms"] * 1e-3), 1)
            e["loss_finite"] = bool(loss == loss and abs(loss) != float("inf"))
            res[m] = e
            g.release()
        res["specaug_over_plain_ms"] = round(res["specaug"]["ms"] / res["plain"]["ms"], 4)
        return res
    finally:
        _lib.set_matmul_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "specaug_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (c), the graphed train steps")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specaug_bench needs a GPU: no timing without one")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters,
           "source_stamp": _lib.source_stamp(),
           "kernels": {name: bench_kernels(a.clips, T, F, pol, a.rounds, a.iters) for name, ((T, F), pol) in SHAPES.items()},
           "train_step_graph": {"batch": a.clips}}
    if not a.no_step:
        for model in STEP_MODELS:
            out["train_step_graph"][model] = {prec: bench_steps(model, a.clips, prec, a.rounds, max(2, a.iters // 5))
                                              for prec in ("fp32", "bf16")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
