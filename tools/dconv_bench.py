"""Dilated-convolution benchmark: writes profiles/dconv_bench.json.

    python tools/dconv_bench.py [--parent-lib PATH/libsrk.so] [--batch 256] [--rounds 7] [--iters 50]

One process, alternating rounds, batch 256, fp32 and bf16:

(a) the two dilated head convolutions of models/model_resnet_dconv.py (384 -> 512 at dilation 4, 512 -> 640 at
    dilation 16; k = 5, L = 500): fwd and bwd (dx + dw + db) through srk_conv1d_nlc_dil_* at their dilation, and
    the SAME shape at dilation 1 (padding 2, so Lo = L: the same FLOPs and kernel families) through the existing
    srk_conv2d_nhwc_fwd16 / _bwd16_acc — on this build ("dil1") and, with --parent-lib, on a second libsrk.so
    built from the parent commit ("parent_dil1"), which is the yardstick: dilation only widens the window of
    input rows a 128-pixel tile touches (128 + 4 -> 128 + 64), so a dilated launch should stay within 1.10 x.
    Each round times every variant once (--iters calls between two device events); the figure is the median
    over rounds, the spread the (max - min) / median of the rounds.
(b) the resnet_dconv train step (forward, loss, backward, Adam) replayed from a HIP graph: utt/s.

Times are device-event times of whole entry-point calls (weight re-layout, 16-bit operand copies, split-K
reductions and bias sums included), not single kernels.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from speechrecognitionproject_amd import _lib, nn as snn  # noqa: E402
from speechrecognitionproject_amd.features import ptr, stream_ptr  # noqa: E402

HEAD = {  # name: L, Ci, Co, K, pad, dil   (model_resnet_dconv.py:99-100)
    "conv2_384x512_d4": (500, 384, 512, 5, 8, 4),
    "conv3_512x640_d16": (500, 512, 640, 5, 32, 16),
}
FUNCS = ("srk_conv2d_workspace_floats", "srk_conv2d_nhwc_fwd16", "srk_conv2d_nhwc_bwd16_acc", "srk_set_option",
         "srk_last_error", "srk_source_stamp", "srk_version")


def load_parent(path):
    """A second libsrk.so (the parent commit's build) beside the package's own, with its own globals."""
    L = ctypes.CDLL(path)
    for name in FUNCS:
        fn = getattr(L, name)
        fn.argtypes = _lib._SIGS[name]
        fn.restype = _lib._RESTYPE.get(name, ctypes.c_int)
    if L.srk_version() != _lib.ABI_VERSION:
        raise SystemExit("--parent-lib: ABI version %d != %d" % (L.srk_version(), _lib.ABI_VERSION))
    return L


def checked(L, name, *args):
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (name, rc, L.srk_last_error().decode(errors="replace")))


def conv_variants(N, shape, parent):
    """{variant: (fwd(), bwd())} closures over preallocated tensors (Lo = L for every variant)."""
    L, Ci, Co, K, pad, dil = shape
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(N, L, Ci, device="cuda", generator=g)
    w = torch.randn(Co, Ci, K, device="cuda", generator=g) / (Ci * K) ** 0.5
    b = torch.randn(Co, device="cuda", generator=g)
    dy = torch.randn(N, L, Co, device="cuda", generator=g)
    y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    ws = torch.empty(Ci * Co * K, device="cuda")
    keep = (x, w, b, dy, y, dx, dw, db, ws)
    here = _lib.lib()

    def dil_fwd():
        checked(here, "srk_conv1d_nlc_dil_fwd", ptr(x), N, L, Ci, ptr(w), ptr(b), Co, K, pad, dil, ptr(y), ptr(ws), None,
                None, stream_ptr())

    def dil_bwd():
        checked(here, "srk_conv1d_nlc_dil_bwd", ptr(x), N, L, Ci, ptr(w), Co, K, pad, dil, ptr(dy), None, ptr(dx),
                ptr(dw), ptr(db), ptr(ws), None, 0, stream_ptr())

    def plain(lib):
        p1 = (K - 1) // 2

        def fwd():
            checked(lib, "srk_conv2d_nhwc_fwd16", ptr(x), N, 1, L, Ci, ptr(w), ptr(b), Co, 1, K, 0, p1, 1, 1, ptr(y),
                    ptr(ws), None, None, stream_ptr())

        def bwd():
            checked(lib, "srk_conv2d_nhwc_bwd16_acc", ptr(x), N, 1, L, Ci, ptr(w), Co, 1, K, 0, p1, 1, 1, ptr(dy), None,
                    ptr(dx), ptr(dw), ptr(db), ptr(ws), None, 0, stream_ptr())
        return fwd, bwd

    out = {"dil": (dil_fwd, dil_bwd), "dil1": plain(here)}
    if parent is not None:
        out["parent_dil1"] = plain(parent)
    return out, keep


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
    return {"ms": round(med, 4), "spread": round((max(samples) - min(samples)) / med, 4), "rounds": len(samples)}


def bench_convs(N, prec, parent, rounds, iters):
    _lib.set_matmul_precision(prec)
    if parent is not None:
        checked(parent, "srk_set_option", b"matmul_precision", _lib.PRECISIONS[prec])
    res = {}
    try:
        for name, shape in HEAD.items():
            variants, keep = conv_variants(N, shape, parent)
            for fwd, bwd in variants.values():   # warm up every variant (code objects, scratch growth)
                for _ in range(3):
                    fwd()
                    bwd()
            torch.cuda.synchronize()
            samples = {(v, d): [] for v in variants for d in ("fwd", "bwd")}
            for _ in range(rounds):
                for v, (fwd, bwd) in variants.items():
                    samples[v, "fwd"].append(time_calls(fwd, iters))
                    samples[v, "bwd"].append(time_calls(bwd, iters))
            L, Ci, Co, K, _, _ = shape
            flops = 2.0 * N * L * Ci * Co * K
            r = {"flops_fwd": flops, "flops_bwd": 2 * flops}
            for (v, d), s in samples.items():
                e = summarize(s)
                e["tflops"] = round((flops if d == "fwd" else 2 * flops) / (e["ms"] * 1e-3) / 1e12, 1)
                r["%s_%s" % (v, d)] = e
            yard = "parent_dil1" if parent is not None else "dil1"
            for d in ("fwd", "bwd"):
                r["ratio_%s_vs_%s" % (d, yard)] = round(r["dil_" + d]["ms"] / r[yard + "_" + d]["ms"], 4)
            res[name] = r
            del variants, keep
    finally:
        _lib.set_matmul_precision("fp32")
        if parent is not None:
            checked(parent, "srk_set_option", b"matmul_precision", 0)
    return res


def bench_step(N, prec, rounds, replays):
    from speechrecognitionproject_amd.graphs import GraphedStep
    from speechrecognitionproject_amd.models import model_resnet_dconv
    from speechrecognitionproject_amd.optim import Adam, FlatParams
    from speechrecognitionproject_amd.synthetic import synthetic_clips
    _lib.set_matmul_precision(prec)
    try:
        torch.manual_seed(0)
        net = model_resnet_dconv.Network().cuda()
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
        samples = [time_calls(g.replay, replays) for _ in range(rounds)]
        loss = float(g.replay().item())
        g.release()
        e = summarize(samples)
        e["utt_per_s"] = round(N / (e["ms"] * 1e-3), 1)
        e["loss_finite"] = bool(loss == loss and abs(loss) != float("inf"))
        return e
    finally:
        _lib.set_matmul_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libsrk.so built from the parent commit (the dilation-1 yardstick)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dconv_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (b), the graphed train step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dconv_bench needs a GPU: no timing without one")
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "rounds": a.rounds, "iters": a.iters,
           "source_stamp": _lib.source_stamp(),
           "parent_source_stamp": parent.srk_source_stamp().decode() if parent is not None else None,
           "convs": {}, "train_step_graph": {}}
    for prec in ("fp32", "bf16"):
        out["convs"][prec] = bench_convs(a.batch, prec, parent, a.rounds, a.iters)
        if not a.no_step:
            out["train_step_graph"][prec] = bench_step(a.batch, prec, a.rounds, max(2, a.iters // 2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
