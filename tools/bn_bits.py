"""Record the bits of the BatchNorm entry points (csrc/bn.hip) of one build of the library.

    SRK_LIB=/path/to/a/trusted/libsrk.so python tools/bn_bits.py --out tests/golden/bn_bits.json

One process records one library (``SRK_LIB``, default: the tree's own libsrk.so); two builds are never loaded into
one process.  tests/test_bn_bits_gpu.py recomputes the same cases with the working tree's library and requires every
digest of the committed record to be equal, so the record is the anchor the kernels are held to from outside the code
under test.  Only entry points that exist since ABI version 3 are used, so an old commit can be recorded.

Shapes (M, C), each the smallest that reaches its path of bn_geom: one quad and one row; the smallest C with a 16-bit
copy; two chunks with the last of one row (RP = 256); two chunks; CQ = 3 (255 of 256 threads live); two channel groups,
the second of one quad; 33 chunks (one past the 32 partials loaded ahead: the clamped tail); 65 chunks; 256 chunks,
the last of one row (the tree form's full width); 8 rows per chunk; 36 rows per chunk (a second, partly masked trip of
the 8-row loop); the same at RP = 16.

Cases per shape; every input is drawn on the host from a seeded generator, the saved statistics, y and the ReLU mask
that a backward reads are formed on the host too, so no case's inputs depend on a kernel:
  * fwd: srk_batchnorm_fwd16_mask in training, relu in {0, 1} x residual in {none, given} x bn_tree in TREES: y, mean,
    invstd, running_mean, running_var, and the mask when relu = 1.  fwd16: the same call (relu, residual) at matmul
    precision bf16 and fp16 with y16 given: y, y16, y16_written.  fwd_eval: eval mode, once.
  * bwd: srk_batchnorm_bwd16_mask in training, relu x residual, each with the mask (and, with relu, y null) and with y:
    dx, dgamma, dbeta, dresidual.  bwd_acc: dgamma_acc / dbeta_acc pre-filled.  bwd_nodx: dx null, dresidual given.
    bwd_eval: eval mode.  bwd16: dx16 and dx16_written at both 16-bit precisions.
  * sync at world in {1, 3}: srk_batchnorm_stats on the ranks' row slices (a rank without rows holds a zero triple),
    srk_batchnorm_combine of those triples, and with its statistics srk_batchnorm_apply, srk_batchnorm_bwd_reduce and
    srk_batchnorm_bwd_dx over all rows.
bn_tree 1 and 2 and the 16-bit cases are taken at WIDE_SHAPES only.

Every output is stored as the sha256 of its raw bytes, which is what the test compares, and every case stores a
digest of its inputs, which tells a drift of the host random number generator from a change of the kernels.  So that
a mismatch can be looked at, an output of up to KEEP_WORDS_UP_TO elements is also stored as its bit patterns: the
whole tensors of the two smallest shapes and the per-channel vectors of the narrow ones.  At 512 elements everywhere
the 256-channel vectors of every case would take the record past the size a committed file may have, so that bound
holds at one wide shape, WORDS_SHAPE, in the bn_tree = 0 forward cases, bwd_acc and the sync cases: every kind of
per-channel vector (statistics, running estimates, gradients and their accumulators, rank sums) is there once.

All these digests go through 1 / sqrtf and expressions the compiler contracts, so the record is bound to the ROCm
install it was made with.  To re-record (a new ROCm, or an intended change of the arithmetic): check out a trusted
commit into a scratch worktree, build it there, and run this script on the GPU with SRK_LIB pointing at that build.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from speechrecognitionproject_amd import _lib  # noqa: E402
from speechrecognitionproject_amd.features import ptr, stream_ptr  # noqa: E402

F32, I64, I32, I16, U8 = torch.float32, torch.int64, torch.int32, torch.int16, torch.uint8
SHAPES = [(1, 4), (3, 8), (257, 4), (255, 8), (1000, 12), (66, 260), (130, 256), (257, 256), (1021, 256), (1027, 256),
          (8200, 256), (33000, 64)]
WIDE_SHAPES = [(3, 8), (130, 256), (1021, 256), (8200, 256)]
WORLDS = [1, 3]
EPS, MOMENTUM = 1e-5, 0.1
KEEP_WORDS_UP_TO = 32
WORDS_SHAPE, KEEP_WORDS_UP_TO_THERE = (130, 256), 512
NOTE = ("Recorded by tools/bn_bits.py from the parent commit of the refactor that gave csrc/bn.hip one reduction plan, "
        "one launcher per reduction and one element launcher.  Every digest goes through 1 / sqrtf and expressions "
        "the compiler contracts, so the record is bound to the ROCm install of the recording.  Re-record: build a "
        "trusted commit in a scratch worktree and run the tool on the GPU with SRK_LIB pointing at that build.")


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(U8).numpy().tobytes())
    return h.hexdigest()


def _record(t, keep):
    t = t.detach().cpu().contiguous().reshape(-1)
    out = {"sha256": _sha(t)}
    if t.numel() <= keep:
        raw = t.view(U8)
        out["bits"] = (raw if t.element_size() == 1 else
                       raw.view(I16).to(I64) & 0xFFFF if t.element_size() == 2 else
                       raw.view(I32).to(I64) & 0xFFFFFFFF).tolist()
    return out


def _case(inputs, outputs, keep=KEEP_WORDS_UP_TO):
    return {"inputs_sha256": _sha(*inputs), "outputs": {k: _record(t, keep) for k, t in outputs.items()}}


def _optr(t):
    return None if t is None else ptr(t)


def _new(*shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device="cuda")


class Inputs:
    """The host-drawn operands of one shape, and the statistics / y / mask a backward reads, formed on the host."""

    def __init__(self, M, C):
        g = torch.Generator().manual_seed(9000 + 131 * M + C)
        self.M, self.C = M, C
        self.x = torch.randn(M, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
        self.gamma = 0.5 + torch.rand(C, generator=g)
        self.beta = torch.randn(C, generator=g) * 0.3
        self.res = torch.randn(M, C, generator=g)
        self.dy = torch.randn(M, C, generator=g)
        self.rm = torch.randn(C, generator=g) * 0.1
        self.rv = 0.5 + torch.rand(C, generator=g)
        self.acc = torch.randn(2, C, generator=g)
        self.mean = self.x.mean(0)
        self.invstd = 1.0 / torch.sqrt(self.x.var(0, unbiased=False) + EPS)
        self.host = [self.x, self.gamma, self.beta, self.res, self.dy, self.rm, self.rv, self.acc, self.mean,
                     self.invstd]
        self.dev = {}

    def y_mask(self, relu, res):
        """The forward's y on the host, and its ReLU bits: bit e of byte i is !(y[4 i + e] <= 0)."""
        y = (self.x - self.mean) * self.invstd * self.gamma + self.beta
        if res:
            y = y + self.res
        if relu:
            y = torch.where(y <= 0, torch.zeros_like(y), y)
        bits = (~(y <= 0)).reshape(-1, 4).to(I32) * torch.tensor([1, 2, 4, 8], dtype=I32)
        return y, bits.sum(1).to(U8)

    def cuda(self, name):
        if name not in self.dev:
            self.dev[name] = getattr(self, name).cuda()
        return self.dev[name]


def _name(kind, inp, tail=""):
    return "%s/M%d_C%d%s" % (kind, inp.M, inp.C, "/" + tail if tail else "")


def forward(inp, relu, res, training=1, y16=False):
    """srk_batchnorm_fwd16_mask at the current options: {output name: tensor}."""
    M, C = inp.M, inp.C
    rm, rv = inp.rm.cuda(), inp.rv.cuda()
    y, mean, invstd = _new(M, C), _new(C), _new(C)
    mask = _new(M * C // 4, dtype=U8) if relu else None
    y16_t = _new(M * C, dtype=I16) if y16 else None
    written = ctypes.c_int(-1)
    _lib.call("srk_batchnorm_fwd16_mask", ptr(inp.cuda("x")), M, C, ptr(inp.cuda("gamma")), ptr(inp.cuda("beta")), EPS,
              MOMENTUM, training, ptr(rm), ptr(rv), ptr(inp.cuda("res")) if res else None, relu, ptr(y), _optr(y16_t),
              ctypes.byref(written), _optr(mask), ptr(mean), ptr(invstd), stream_ptr())
    torch.cuda.synchronize()
    out = {"y": y, "mean": mean, "invstd": invstd, "running_mean": rm, "running_var": rv}
    if relu:
        out["mask"] = mask
    if y16:
        out = {"y": y, "y16": y16_t, "y16_written": torch.tensor([written.value], dtype=I32)}
    return out


def backward(inp, relu, res, by_mask, training=1, acc=False, dx=True, dx16=False):
    """srk_batchnorm_bwd16_mask at the current options: (extra host inputs, {output name: tensor})."""
    M, C = inp.M, inp.C
    y_h, mask_h = inp.y_mask(relu, res)
    y = None if (relu and by_mask) else y_h.cuda()
    mask = mask_h.cuda() if by_mask else None
    dx_t = _new(M, C) if dx else None
    dres = _new(M, C) if res else None
    dgamma, dbeta = _new(C), _new(C)
    accs = inp.acc.cuda() if acc else None
    dx16_t = _new(M * C, dtype=I16) if dx16 else None
    written = ctypes.c_int(-1)
    _lib.call("srk_batchnorm_bwd16_mask", ptr(inp.cuda("x")), _optr(y), _optr(mask), ptr(inp.cuda("dy")), M, C,
              ptr(inp.cuda("gamma")), ptr(inp.cuda("mean")), ptr(inp.cuda("invstd")), training, relu, _optr(dx_t),
              _optr(dx16_t), ctypes.byref(written), ptr(dgamma), ptr(dbeta), _optr(dres),
              ptr(accs[0]) if acc else None, ptr(accs[1]) if acc else None, stream_ptr())
    torch.cuda.synchronize()
    out = {"dgamma": dgamma, "dbeta": dbeta}
    if dx:
        out["dx"] = dx_t
    if res:
        out["dresidual"] = dres
    if acc:
        out["dgamma_acc"], out["dbeta_acc"] = accs[0], accs[1]
    if dx16:
        out["dx16"], out["dx16_written"] = dx16_t, torch.tensor([written.value], dtype=I32)
    return [y_h, mask_h], out


def sync(inp, world):
    """The SyncBatchNorm pieces: the ranks' triples from row slices, their combination, and apply / bwd_reduce /
    bwd_dx over all rows with the combined statistics (relu and residual on)."""
    M, C = inp.M, inp.C
    x, dy, res = inp.cuda("x"), inp.cuda("dy"), inp.cuda("res")
    allst = torch.zeros((world, 3 * C), device="cuda")
    for r in range(world):
        lo, hi = M * r // world, M * (r + 1) // world
        if hi > lo:
            _lib.call("srk_batchnorm_stats", ptr(x[lo:hi]), hi - lo, C, ptr(allst[r]), stream_ptr())
    rm, rv = inp.rm.cuda(), inp.rv.cuda()
    mean, invstd, total = _new(C), _new(C), _new(1)
    _lib.call("srk_batchnorm_combine", ptr(allst), world, C, EPS, MOMENTUM, ptr(rm), ptr(rv), ptr(mean), ptr(invstd),
              ptr(total), stream_ptr())
    y = _new(M, C)
    _lib.call("srk_batchnorm_apply", ptr(x), M, C, ptr(mean), ptr(invstd), ptr(inp.cuda("gamma")),
              ptr(inp.cuda("beta")), ptr(res), 1, ptr(y), stream_ptr())
    sums = _new(2 * C)
    _lib.call("srk_batchnorm_bwd_reduce", ptr(x), ptr(y), ptr(dy), M, C, ptr(mean), ptr(invstd), 1, ptr(sums),
              stream_ptr())
    dx, dres = _new(M, C), _new(M, C)
    _lib.call("srk_batchnorm_bwd_dx", ptr(x), ptr(y), ptr(dy), M, C, ptr(total), ptr(inp.cuda("gamma")), ptr(mean),
              ptr(invstd), ptr(sums), 1, ptr(dx), ptr(dres), stream_ptr())
    torch.cuda.synchronize()
    return {"stats": allst, "mean": mean, "invstd": invstd, "running_mean": rm, "running_var": rv, "total": total,
            "y": y, "sums": sums, "dx": dx, "dresidual": dres}


def shape_cases(M, C):
    inp = Inputs(M, C)
    wide = (M, C) in WIDE_SHAPES
    more = KEEP_WORDS_UP_TO_THERE if (M, C) == WORDS_SHAPE else KEEP_WORDS_UP_TO
    out = {}
    for tree in ((0, 1, 2) if wide else (0,)):
        with _lib.options(bn_tree=tree):
            for relu in (0, 1):
                for res in (0, 1):
                    out[_name("fwd", inp, "relu%d_res%d_tree%d" % (relu, res, tree))] = _case(
                        inp.host, forward(inp, relu, res), more if tree == 0 else KEEP_WORDS_UP_TO)
    out[_name("fwd_eval", inp)] = _case(inp.host, forward(inp, 1, 1, training=0))
    for relu in (0, 1):
        for res in (0, 1):
            for by_mask in (1, 0):
                extra, got = backward(inp, relu, res, by_mask)
                out[_name("bwd", inp, "relu%d_res%d_%s" % (relu, res, "mask" if by_mask else "y"))] = _case(
                    inp.host + extra, got)
    for kind, kw in (("bwd_acc", {"acc": True}), ("bwd_nodx", {"dx": False}), ("bwd_eval", {"training": 0})):
        extra, got = backward(inp, 1, 1, 1, **kw)
        out[_name(kind, inp)] = _case(inp.host + extra, got, more if kind == "bwd_acc" else KEEP_WORDS_UP_TO)
    if wide:
        assert C % 8 == 0
        for prec in ("bf16", "fp16"):
            with _lib.options(matmul_precision=_lib.PRECISIONS[prec]):
                out[_name("fwd16", inp, prec)] = _case(inp.host, forward(inp, 1, 1, y16=True))
                extra, got = backward(inp, 1, 1, 1, dx16=True)
                out[_name("bwd16", inp, prec)] = _case(inp.host + extra, got)
    for world in WORLDS:
        out[_name("sync", inp, "world%d" % world)] = _case(inp.host, sync(inp, world), more)
    return out


def case_count():
    """Cases per shape: 4 forward + eval, 8 backward + acc / nodx / eval, 2 sync; at a wide shape 8 more forward (two
    more trees) and 2 + 2 at 16 bits."""
    return len(SHAPES) * (5 + 11 + len(WORLDS)) + len(WIDE_SHAPES) * (8 + 4)


def compute():
    """{case name: {"inputs_sha256", "outputs": {name: {"sha256", ["bits"]}}}} of the loaded library."""
    cases = {}
    for M, C in SHAPES:
        cases.update(shape_cases(M, C))
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
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "bn_bits.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_bits needs a GPU: the bits are the kernels'")
    rec = {"note": NOTE, "source_stamp": _lib.source_stamp(),
           "device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "cases": compute()}
    assert len(rec["cases"]) == case_count()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write_record(rec, a.out)
    print("recorded %d cases from %s (source stamp %s) into %s" % (len(rec["cases"]), _lib.LIB_PATH,
                                                                   rec["source_stamp"], a.out))


if __name__ == "__main__":
    main()
