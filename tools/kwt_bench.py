"""Transformer-encoder kernels / fbanks_kwt benchmark: writes profiles/kwt_bench.json.

    python tools/kwt_bench.py [--rounds 7] [--iters 20] [--batch 512] [--parent-tree DIR]

One process, alternating rounds (every variant timed once per round, --iters calls between two device events; the
figure is the median over rounds, the spread (max - min) / median), fp32 tensors:

(a) the attention core srk_mhsa_fwd / _bwd at (B, H, T, dh) = (batch, 1, 98, 64) and (batch, 3, 98, 64) with the
    achieved GFLOP/s over the algorithmic flops (forward 4 B H T^2 dh, backward 10 B H T^2 dh) and GB/s over the
    algorithmic bytes, next to the torch spelling softmax(q k^T scale) v in fp32 (forward, and autograd backward of
    all three gradients) and F.scaled_dot_product_attention on the same [B, H, T, dh] views;
(b) srk_layernorm_fwd / _bwd on [batch * 98, 64] and [batch * 98, 192] with the fused residual, next to F.layer_norm
    (the residual add included, forward and autograd backward) and a plain ``copy_`` of the same byte count;
(c) srk_gelu_fwd / _bwd on batch * 98 * 256 elements next to F.gelu and a copy of the same byte count;
(d) the fbanks_kwt (KWT-1) train step (forward, loss, backward, Adam) replayed from a HIP graph next to fbanks_cnn's
    and fbanks_dscnn's at the same batch, in fp32 and bf16: ms per step and utt/s, with the eager step's per-category
    kernel times and each category's share of their sum;
(e) with --parent-tree DIR (a built checkout of the parent commit): ``python bench.py --gpus 1`` run in child
    processes from DIR and from this tree alternately, --bench-runs times each, both result lines recorded.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

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
    return {"us": round(med * 1e3, 2), "spread": round((max(samples) - min(samples)) / med, 4), "rounds": len(samples)}


def run_variants(variants, rounds):
    """variants: name -> (call, algorithmic bytes or None, algorithmic flops or None, iterations)."""
    for call, _, _, _ in variants.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (call, _, _, it) in variants.items():
            samples[v].append(time_calls(call, it))
    res = {}
    for v, (_, nbytes, flops, _) in variants.items():
        e = summarize(samples[v])
        if nbytes:
            e["bytes"] = nbytes
            e["gb_per_s"] = round(nbytes / (e["us"] * 1e-6) / 1e9, 1)
        if flops:
            e["flops"] = flops
            e["gflop_per_s"] = round(flops / (e["us"] * 1e-6) / 1e9, 1)
        res[v] = e
    return res


def copy_call(nbytes):
    n = int(nbytes // 8)
    src = torch.empty(n, device="cuda").normal_()
    dst = torch.empty(n, device="cuda")
    return lambda: dst.copy_(src)


def bench_attention(B, H, T, dh, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(1)
    D, scale = H * dh, dh ** -0.5
    qkv = torch.randn(B, T, 3 * D, device="cuda", generator=g)
    do = torch.randn(B, T, D, device="cuda", generator=g)
    o, lse, dqkv = torch.empty_like(do), torch.empty(B, H, T, device="cuda"), torch.empty_like(qkv)

    def fwd():
        _lib.call("srk_mhsa_fwd", ptr(qkv), B, H, T, dh, scale, ptr(o), ptr(lse), stream_ptr())

    def bwd():
        _lib.call("srk_mhsa_bwd", ptr(qkv), ptr(lse), ptr(do), B, H, T, dh, scale, ptr(dqkv), stream_ptr())

    # torch on [B, H, T, dh] views of the same memory
    q, k, v = (t.reshape(B, T, H, dh).transpose(1, 2).detach().requires_grad_(True) for t in qkv.split(D, dim=2))
    g4 = do.reshape(B, T, H, dh).transpose(1, 2)
    state = {}

    def torch_fwd():
        state["o"] = torch.softmax((q @ k.transpose(2, 3)) * scale, dim=3) @ v

    def torch_bwd():
        torch.autograd.grad(state["o"], (q, k, v), g4, retain_graph=True)

    def sdpa_fwd():
        state["s"] = F.scaled_dot_product_attention(q, k, v)

    def sdpa_bwd():
        torch.autograd.grad(state["s"], (q, k, v), g4, retain_graph=True)

    n = float(B) * T * D
    b_fwd, b_bwd = 4.0 * (4 * n + B * H * T), 4.0 * (7 * n + B * H * T)
    f_fwd, f_bwd = 4.0 * B * H * T * T * dh, 10.0 * B * H * T * T * dh
    slow = max(2, iters // 4)
    variants = {"fwd": (fwd, b_fwd, f_fwd, iters), "bwd": (bwd, b_bwd, f_bwd, iters),
                "torch_softmax_fwd": (torch_fwd, b_fwd, f_fwd, slow), "torch_softmax_bwd": (torch_bwd, b_bwd, f_bwd, slow),
                "torch_sdpa_fwd": (sdpa_fwd, b_fwd, f_fwd, slow), "torch_sdpa_bwd": (sdpa_bwd, b_bwd, f_bwd, slow)}
    fwd()
    torch_fwd()
    res = run_variants(variants, rounds)
    fwd()
    torch_fwd()
    torch.cuda.synchronize()
    ref = state["o"].detach().transpose(1, 2).reshape(B, T, D)
    res["fwd_vs_torch_rel_err"] = float((o - ref).abs().max() / ref.abs().max())
    res["shape"] = {"B": B, "H": H, "T": T, "dh": dh}
    return res


def bench_layernorm(M, D, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(2)
    x, r, dy = (torch.randn(M, D, device="cuda", generator=g) for _ in range(3))
    gamma, beta = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    y, ds = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    dgamma, dbeta = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    ws = torch.empty(int(_lib.lib().srk_layernorm_workspace_floats(M, D)), device="cuda")

    def fwd():
        _lib.call("srk_layernorm_fwd", ptr(x), ptr(r), ptr(gamma), ptr(beta), M, D, 1e-5, ptr(y), ptr(mean), ptr(rstd),
                  stream_ptr())

    def bwd():
        _lib.call("srk_layernorm_bwd", ptr(x), ptr(r), ptr(gamma), ptr(mean), ptr(rstd), ptr(dy), M, D, ptr(ds),
                  ptr(dgamma), ptr(dbeta), 0.0, ptr(ws), stream_ptr())

    xt, rt = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    state = {}

    def torch_fwd():
        state["y"] = F.layer_norm(xt + rt, (D,), gt, bt, 1e-5)

    def torch_bwd():
        torch.autograd.grad(state["y"], (xt, rt, gt, bt), dy, retain_graph=True)

    b_fwd = 4.0 * (3.0 * M * D + 2 * D + 2 * M)
    b_bwd = 4.0 * (4.0 * M * D + 3 * D + 2 * M)
    variants = {"fwd": (fwd, b_fwd, None, iters), "bwd": (bwd, b_bwd, None, iters),
                "copy_fwd_bytes": (copy_call(b_fwd), b_fwd, None, iters),
                "copy_bwd_bytes": (copy_call(b_bwd), b_bwd, None, iters),
                "torch_fwd": (torch_fwd, b_fwd, None, iters), "torch_bwd": (torch_bwd, b_bwd, None, max(2, iters // 2))}
    fwd()
    torch_fwd()
    res = run_variants(variants, rounds)
    res["fwd_over_copy_bw"] = round(res["fwd"]["gb_per_s"] / res["copy_fwd_bytes"]["gb_per_s"], 3)
    res["bwd_over_copy_bw"] = round(res["bwd"]["gb_per_s"] / res["copy_bwd_bytes"]["gb_per_s"], 3)
    res["shape"] = [M, D]
    return res


def bench_gelu(n, rounds, iters):
    g = torch.Generator(device="cuda").manual_seed(3)
    x, dy = torch.randn(n, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    xt = x.clone().requires_grad_(True)
    state = {}

    def torch_fwd():
        state["y"] = F.gelu(xt)

    variants = {
        "fwd": (lambda: _lib.call("srk_gelu_fwd", ptr(x), n, ptr(y), stream_ptr()), 8.0 * n, None, iters),
        "bwd": (lambda: _lib.call("srk_gelu_bwd", ptr(x), ptr(dy), n, ptr(dx), stream_ptr()), 12.0 * n, None, iters),
        "copy_fwd_bytes": (copy_call(8.0 * n), 8.0 * n, None, iters),
        "copy_bwd_bytes": (copy_call(12.0 * n), 12.0 * n, None, iters),
        "torch_fwd": (torch_fwd, 8.0 * n, None, iters),
        "torch_bwd": (lambda: torch.autograd.grad(state["y"], xt, dy, retain_graph=True), 12.0 * n, None, iters),
    }
    torch_fwd()
    res = run_variants(variants, rounds)
    res["fwd_over_copy_bw"] = round(res["fwd"]["gb_per_s"] / res["copy_fwd_bytes"]["gb_per_s"], 3)
    res["bwd_over_copy_bw"] = round(res["bwd"]["gb_per_s"] / res["copy_bwd_bytes"]["gb_per_s"], 3)
    res["n"] = n
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
    """{category: ms} of one eager step (the library's per-launch event timers) and each category's share."""
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
    total = sum(by.values()) or 1.0
    order = sorted(by.items(), key=lambda kv: -kv[1])
    return {k: round(v, 4) for k, v in order}, {k: round(v / total, 4) for k, v in order}


MODELS = ("fbanks_kwt", "fbanks_cnn", "fbanks_dscnn")


def bench_steps(N, prec, rounds, replays):
    from speechrecognitionproject_amd.graphs import GraphedStep
    _lib.set_matmul_precision(prec)
    try:
        res, graphs, bodies = {}, {}, {}
        # every eager pass first: the library's grow-only scratch buffers reach every model's size before a capture
        for m in MODELS:
            bodies[m] = make_step(m, N)
            ms, share = eager_kernel_times(bodies[m])
            res[m] = {"eager_kernel_ms": ms, "eager_kernel_share": share}
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
        return res
    finally:
        _lib.set_matmul_precision("fp32")


def bench_py_ab(parent, runs, steps, warmup, timeout):
    """bench.py's own result line from the parent tree and from this one, alternating, a child process each."""
    out = {"parent": [], "this": [], "args": ["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]}
    for _ in range(runs):
        for tag, tree in (("parent", parent), ("this", REPO)):
            try:
                r = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + out["args"], cwd=tree,
                                   capture_output=True, text=True, timeout=timeout)
            except subprocess.TimeoutExpired:
                out[tag].append({"error": "not finished within %d s" % timeout})
                return out
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                out[tag].append({"error": r.returncode, "stderr_tail": r.stderr[-400:]})
                return out      # nothing more is started after a failed run
            line = json.loads(lines[-1])
            out[tag].append({k: line.get(k) for k in ("metric", "value", "unit") if k in line})
    vals = {t: [e["value"] for e in out[t]] for t in ("parent", "this")}
    out["median"] = {t: statistics.median(v) for t, v in vals.items()}
    out["spread"] = {t: round((max(v) - min(v)) / statistics.median(v), 4) for t, v in vals.items()}
    out["this_over_parent"] = round(out["median"]["this"] / out["median"]["parent"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kwt_bench.json"))
    ap.add_argument("--no-step", action="store_true", help="skip (d), the graphed train steps")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: run (e)")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--bench-timeout", type=int, default=600, help="seconds allowed to one bench.py run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kwt_bench needs a GPU: no timing without one")
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "batch": a.batch,
           "source_stamp": _lib.source_stamp(), "attention": {}, "layernorm": {}, "train_step_graph": {"batch": a.batch}}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")

    for H in (1, 3):
        out["attention"]["h%d" % H] = bench_attention(a.batch, H, 98, 64, a.rounds, a.iters)
        torch.cuda.empty_cache()
    for D in (64, 192):
        out["layernorm"]["d%d" % D] = bench_layernorm(a.batch * 98, D, a.rounds, a.iters)
        torch.cuda.empty_cache()
    out["gelu"] = bench_gelu(a.batch * 98 * 256, a.rounds, a.iters)
    torch.cuda.empty_cache()
    save()
    if not a.no_step:
        for prec in ("fp32", "bf16"):
            out["train_step_graph"][prec] = bench_steps(a.batch, prec, a.rounds, max(2, a.iters // 4))
            save()
    if a.parent_tree:
        torch.cuda.synchronize()
        out["bench_py_parent_vs_this"] = bench_py_ab(os.path.abspath(a.parent_tree), a.bench_runs, a.bench_steps,
                                                     a.bench_warmup, a.bench_timeout)
    else:
        out["bench_py_parent_vs_this"] = "not measured (no --parent-tree)"
    save()
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
