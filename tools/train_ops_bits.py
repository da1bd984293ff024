"""Record the bits of the training-step ops (Adam, cross-entropy, dropout mask) of one build of the library.

    SRK_LIB=/path/to/a/trusted/libsrk.so python tools/train_ops_bits.py --out tests/golden/train_ops_bits.json

One process records one library (``SRK_LIB``, default: the tree's own libsrk.so); two builds are never loaded into
one process.  tests/test_train_ops_bits_gpu.py recomputes the same cases with the working tree's library and requires
every digest of the committed record to be equal, so the record is the anchor the kernels are held to from outside
the code under test.  Only entry points that exist since ABI version 3 are used, so an old commit can be recorded.

Cases
  * Adam, n in BITS_N (every tail length of the float4 loop, and one n past a grid stride), 4 steps, the inputs and
    hyper-parameters of tests/test_optim_ext_gpu.py, grad_scale 0.5: srk_adam_step_state; srk_adam_step_scaled (scale
    1024, growth interval 2, an inf in the third gradient at n // 2); srk_adam_step (host lr, steps 1..4);
    srk_adamw_step with everything off, with the clip on at 1e30, and with decay (alternate 64-float chunks marked),
    clipping at 0.01 and an EMA at 0.9 all on.
  * Cross-entropy, (B, C) in CE_SHAPES: srk_cross_entropy, and srk_cross_entropy_mix with a partner / lam draw and
    smoothing 0.1: loss and dlogits.
  * Dropout mask, n in DROPOUT_N, p = 0.5: srk_dropout_fwd and srk_dropout_fwd_state: y, keep (and the state).

Every output is stored as the sha256 of its raw bytes, which is what the test compares.  So that a mismatch can be
looked at, an output of up to 512 elements is also stored as its uint32 bit patterns (bytes for the uint8 mask), and
one of up to 1027 elements as its first and last 16 words: for the Adam buffers at n = 1026 and 1027 that is the
start of the float4 body and the whole scalar tail, which is where the code paths differ; all 1027 words of each of
the 38 such buffers would make the record half a megabyte instead of a few tens of kilobytes.  Every case also stores
a digest of its inputs, which tells a drift of the host random number generator from a change of the kernels.

The Adam and dropout digests hold under any toolchain: every rounding of the update is explicit, and the compiler's
default fp32 division and square root are correctly rounded.  The cross-entropy digests go through expf / logf and are
bound to the ROCm install the record was made with.  To re-record (a new ROCm, or an intended change of the
arithmetic): check out a trusted commit into a scratch worktree, build it there, and run this script on the GPU with
SRK_LIB pointing at that build.
"""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from speechrecognitionproject_amd import _lib  # noqa: E402
from speechrecognitionproject_amd.features import ptr, stream_ptr  # noqa: E402

F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8
BITS_N = [1, 5, 1026, 1027, 2099201]      # tests/test_optim_ext_gpu.py's BITS_N
STEPS = 4
LR, B1, B2, EPS, GS = 1e-3, 0.9, 0.999, 1e-8, 0.5
CE_SHAPES = [(1, 1), (5, 12), (7, 65), (4, 257)]
DROPOUT_N = [1, 257]
KEEP_ARRAYS_UP_TO = 1027    # elements: beyond, the digest alone
KEEP_WHOLE_UP_TO = 512      # elements: up to here every word, beyond the first and last WINDOW words
WINDOW = 16
NOTE = ("Recorded by tools/train_ops_bits.py from the parent commit of the refactor that left one Adam update, one "
        "cross-entropy row kernel and one mask body.  The adam* and dropout* digests hold under any toolchain (every "
        "rounding is explicit, fp32 division and sqrt are correctly rounded); the ce* digests go through expf / logf "
        "and are bound to the ROCm install of the recording.  Re-record: build a trusted commit in a scratch "
        "worktree and run the tool on the GPU with SRK_LIB pointing at that build.")


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(U8).numpy().tobytes())
    return h.hexdigest()


def _record(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    out = {"sha256": _sha(t)}
    if t.numel() <= KEEP_ARRAYS_UP_TO:
        raw = t.view(U8)
        words = (raw if t.element_size() == 1 else raw.view(I32).to(I64) & 0xFFFFFFFF).tolist()
        if t.numel() <= KEEP_WHOLE_UP_TO:
            out["bits"] = words
        else:
            out["head"], out["tail"] = words[:WINDOW], words[-WINDOW:]
    return out


def _case(inputs, outputs):
    return {"inputs_sha256": _sha(*inputs), "outputs": {k: _record(t) for k, t in outputs.items()}}


# ---------------------------------------------------------------- Adam
def adam_inputs(n):
    """tests/test_optim_ext_gpu.py's _inputs(n)."""
    g = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.01
    v0 = (torch.randn(n, generator=g) * 0.01).abs()
    grads = [torch.randn(n, generator=g) for _ in range(STEPS)]
    return p0, m0, v0, grads


def _adam_state():
    st = torch.zeros(8, dtype=F32)
    st[4] = LR
    return st.view(I64).cuda()


def _optr(t):
    return None if t is None else ptr(t)


def _adamw(p, g, m, v, st, scaler=None, wd=0.0, mask=None, max_norm=0.0, clip=None, ema=None, d=0.0, ws=None):
    _lib.call("srk_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), B1, B2, EPS, ptr(st), GS, _optr(scaler), wd,
              _optr(mask), max_norm, _optr(clip), _optr(ema), d, _optr(ws), stream_ptr())


def adam_cases(n):
    p0, m0, v0, grads = adam_inputs(n)
    scaled = [g * 1024.0 for g in grads]
    scaled[2][n // 2] = float("inf")
    mask0 = (torch.arange((n + 63) // 64) % 2 == 0).to(U8)
    out = {}

    def run(name, step, grads=grads, extra_in=(), **extra_out):
        p, m, v, st = p0.cuda(), m0.cuda(), v0.cuda(), _adam_state()
        for k, g in enumerate(grads):
            step(p, g.cuda(), m, v, st, k + 1)
        torch.cuda.synchronize()
        res = {"param": p, "exp_avg": m, "exp_avg_sq": v, "state": st}
        res.update(extra_out)
        out["%s/n%d" % (name, n)] = _case([p0, m0, v0, *grads, *extra_in], res)

    run("adam_state", lambda p, g, m, v, st, k: _lib.call(
        "srk_adam_step_state", ptr(p), ptr(g), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), GS, stream_ptr()))
    sc = torch.zeros(8, dtype=I32, device="cuda")
    _lib.call("srk_grad_scaler_init", ptr(sc), 1024.0, 2.0, 0.5, 2, stream_ptr())
    run("adam_scaled", lambda p, g, m, v, st, k: _lib.call(
        "srk_adam_step_scaled", ptr(p), ptr(g), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), GS, ptr(sc), stream_ptr()),
        grads=scaled, scaler=sc)
    run("adam_host", lambda p, g, m, v, st, k: _lib.call(
        "srk_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), n, LR, B1, B2, EPS, k, GS, stream_ptr()))
    run("adamw_off", lambda p, g, m, v, st, k: _adamw(p, g, m, v, st))
    ws = torch.empty(int(_lib.lib().srk_adamw_workspace_floats(n)), dtype=F32, device="cuda")
    clip = torch.zeros(4, dtype=I32, device="cuda")
    run("adamw_clip_1e30", lambda p, g, m, v, st, k: _adamw(p, g, m, v, st, max_norm=1e30, clip=clip, ws=ws),
        clip_state=clip)
    clip2, ema, mask = torch.zeros(4, dtype=I32, device="cuda"), p0.cuda().clone(), mask0.cuda()
    run("adamw_all_on", lambda p, g, m, v, st, k: _adamw(p, g, m, v, st, wd=1e-2, mask=mask, max_norm=0.01, clip=clip2,
                                                        ema=ema, d=0.9, ws=ws),
        extra_in=(mask0,), clip_state=clip2, ema=ema)
    return out


# ---------------------------------------------------------------- cross-entropy
def ce_cases(B, C):
    g = torch.Generator().manual_seed(4000 + 1000 * B + C)
    logits = torch.randn(B, C, generator=g) * 3.0
    labels = torch.randint(0, C, (B,), generator=g, dtype=I64)
    partner = torch.randperm(B, generator=g).to(I32)
    lam = torch.rand(B, generator=g)
    x, y, pt, lm = logits.cuda(), labels.cuda(), partner.cuda(), lam.cuda()
    out = {}
    for name, mix in (("ce", False), ("ce_mix", True)):
        loss = torch.empty((), device="cuda")
        dx, ws = torch.empty_like(x), torch.empty(B + 1, device="cuda")
        if mix:
            _lib.call("srk_cross_entropy_mix", ptr(x), ptr(y), ptr(pt), ptr(lm), B, C, 0.1, ptr(loss), ptr(dx), ptr(ws),
                      stream_ptr())
        else:
            _lib.call("srk_cross_entropy", ptr(x), ptr(y), B, C, ptr(loss), ptr(dx), ptr(ws), stream_ptr())
        torch.cuda.synchronize()
        out["%s/B%d_C%d" % (name, B, C)] = _case([logits, labels, partner, lam], {"loss": loss, "dlogits": dx})
    return out


# ---------------------------------------------------------------- dropout mask
def dropout_cases(n):
    import ctypes
    x0 = torch.randn(n, generator=torch.Generator().manual_seed(7000 + n))
    x = x0.cuda()
    out = {}
    y, keep = torch.empty_like(x), torch.empty(n, dtype=U8, device="cuda")
    _lib.call("srk_dropout_fwd", ptr(x), n, 0.5, ctypes.c_uint64(0x5EED0123456789AB), ptr(y), ptr(keep), stream_ptr())
    torch.cuda.synchronize()
    out["dropout_fwd/n%d" % n] = _case([x0], {"y": y, "keep": keep})
    st0 = torch.tensor([77, 3], dtype=I64)              # [base, counter]
    st = st0.cuda()
    y, keep = torch.empty_like(x), torch.empty(n, dtype=U8, device="cuda")
    _lib.call("srk_dropout_fwd_state", ptr(x), n, 0.5, ptr(st), ptr(y), ptr(keep), stream_ptr())
    torch.cuda.synchronize()
    out["dropout_fwd_state/n%d" % n] = _case([x0, st0], {"y": y, "keep": keep, "state": st})
    return out


def compute():
    """{case name: {"inputs_sha256", "outputs": {name: {"sha256", ["bits"]}}}} of the loaded library."""
    cases = {}
    for n in BITS_N:
        cases.update(adam_cases(n))
    for B, C in CE_SHAPES:
        cases.update(ce_cases(B, C))
    for n in DROPOUT_N:
        cases.update(dropout_cases(n))
    return cases


def write_record(rec, path):
    """JSON with one case per line, so that a re-recording shows as a diff of the cases that changed."""
    head = {k: v for k, v in rec.items() if k != "cases"}
    with open(path, "w") as f:
        f.write(json.dumps(head, sort_keys=True, indent=1)[:-2] + ',\n "cases": {\n')
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(c, sort_keys=True, separators=(",", ":")))
                           for k, c in sorted(rec["cases"].items())))
        f.write("\n }\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "train_ops_bits.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_ops_bits needs a GPU: the bits are the kernels'")
    rec = {"note": NOTE, "source_stamp": _lib.source_stamp(),
           "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cases": compute()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write_record(rec, a.out)
    print("recorded %d cases from %s (source stamp %s) into %s" % (len(rec["cases"]), _lib.LIB_PATH,
                                                                   rec["source_stamp"], a.out))


if __name__ == "__main__":
    main()
