"""srk_adamw_step and optim.Adam's extensions on the GPU: AdamW decay, global-norm clipping, the weight EMA.

With the features off (or the clip on but not active) the new entry is held to srk_adam_step_state /
srk_adam_step_scaled bit for bit; the norm to float64 within a bound derived from the kernel's summation shape; the
whole step to CPU torch; the skip, the guard bands, the captured step, ema_weights() and the command line follow.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import optim_oracle as O
from guarded import WS_BYTES, Arena, Guarded, same_bits
from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import nn as snn
from speechrecognitionproject_amd.features import ptr, stream_ptr
from speechrecognitionproject_amd.optim import Adam, FlatParams, LossScaler

pytestmark = pytest.mark.gpu

F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8
# test_guard_bands_gpu.py's ADAM_N plus 1026: the old kernel's scalar tail rounds a pair of elements (n % 4 >= 2)
# differently from a last single one, and the new kernel mirrors that, so a two-element tail is a path of its own.
# 2099201 is past one grid stride of both kernels (2048 x 256 x 4 floats for the update, 1024 x 256 x 4 for the norm:
# its lanes take up to three trips).
BITS_N = [1, 5, 1026, 1027, 2099201]
STEPS = 4
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _optr(t):
    return None if t is None else ptr(t)


def _adam_state(lr=LR):
    st = torch.zeros(8, dtype=F32)
    st[4] = lr
    return st.view(I64).cuda()


def _scaler(scale=1024.0, interval=2):
    sc = torch.zeros(8, dtype=I32, device="cuda")
    _lib.call("srk_grad_scaler_init", ptr(sc), scale, 2.0, 0.5, interval, stream_ptr())
    return sc


def _ws(n):
    return torch.empty(int(_lib.lib().srk_adamw_workspace_floats(n)), dtype=F32, device="cuda")


def adamw(p, g, m, v, st, gs=1.0, scaler=None, wd=0.0, mask=None, max_norm=0.0, clip=None, ema=None, d=0.0, ws=None):
    _lib.call("srk_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), B1, B2, EPS, ptr(st), gs, _optr(scaler), wd,
              _optr(mask), max_norm, _optr(clip), _optr(ema), d, _optr(ws), stream_ptr())


def _inputs(n, seed=0):
    g = torch.Generator().manual_seed(1000 + n + seed)
    p0 = torch.randn(n, generator=g)
    m0 = torch.randn(n, generator=g) * 0.01
    v0 = (torch.randn(n, generator=g) * 0.01).abs()
    grads = [torch.randn(n, generator=g) for _ in range(STEPS)]
    return p0, m0, v0, grads


def _clip_floats(clip):
    return clip.view(F32)[:2].tolist()


# ---------------------------------------------------------------- 5, 6: the old entry points' bits
@functools.lru_cache(maxsize=None)
def _old_state_run(n):
    """STEPS steps of srk_adam_step_state at grad_scale 0.5: p, m, v, state after the last (computed once)."""
    p0, m0, v0, grads = _inputs(n)
    p, m, v, st = p0.cuda(), m0.cuda(), v0.cuda(), _adam_state()
    for g in grads:
        _lib.call("srk_adam_step_state", ptr(p), ptr(g.cuda()), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), 0.5,
                  stream_ptr())
    torch.cuda.synchronize()
    return p, m, v, st


@pytest.mark.parametrize("n", BITS_N)
def test_features_off_is_adam_step_state(gpu, n):
    p0, m0, v0, grads = _inputs(n)
    p, m, v, st = p0.cuda(), m0.cuda(), v0.cuda(), _adam_state()
    for g in grads:
        adamw(p, g.cuda(), m, v, st, gs=0.5)
    torch.cuda.synchronize()
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "state"), (p, m, v, st), _old_state_run(n)):
        assert same_bits(a, b), "%s differs from srk_adam_step_state's at n = %d" % (name, n)
    assert int(st[0]) == STEPS


@pytest.mark.parametrize("n", BITS_N)
def test_features_off_is_adam_step_scaled(gpu, n):
    """With a scaler (scale 1024, growing after 2 clean steps), the third step's gradient holding an inf."""
    p0, m0, v0, grads = _inputs(n)
    grads = [g * 1024.0 for g in grads]
    grads[2][n // 2] = float("inf")
    runs = []
    for new in (False, True):
        p, m, v, st, sc = p0.cuda(), m0.cuda(), v0.cuda(), _adam_state(), _scaler()
        for g in grads:
            if new:
                adamw(p, g.cuda(), m, v, st, gs=0.5, scaler=sc)
            else:
                _lib.call("srk_adam_step_scaled", ptr(p), ptr(g.cuda()), ptr(m), ptr(v), n, B1, B2, EPS, ptr(st), 0.5,
                          ptr(sc), stream_ptr())
        torch.cuda.synchronize()
        runs.append((p, m, v, st, sc))
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "state", "scaler"), runs[1], runs[0]):
        assert same_bits(a, b), "%s differs from srk_adam_step_scaled's at n = %d" % (name, n)
    st, sc = runs[1][3], runs[1][4]
    assert int(st[0]) == STEPS - 1 and int(sc[7]) == 1              # one step skipped, counted
    assert sc.view(F32)[0].item() == 1024.0                         # grew after two clean steps, halved on the inf


@pytest.mark.parametrize("n", BITS_N)
def test_clip_on_but_inactive_keeps_the_bits(gpu, n):
    p0, m0, v0, grads = _inputs(n)
    p, m, v, st = p0.cuda(), m0.cuda(), v0.cuda(), _adam_state()
    clip, ws = torch.zeros(4, dtype=I32, device="cuda"), _ws(n)
    for g in grads:
        adamw(p, g.cuda(), m, v, st, gs=0.5, max_norm=1e30, clip=clip, ws=ws)
        assert clip.view(F32)[1].item() == 1.0                      # exactly 1.0f
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "state"), (p, m, v, st), _old_state_run(n)):
        assert same_bits(a, b), "%s differs from srk_adam_step_state's at n = %d" % (name, n)
    assert clip[2].item() == 0 and clip[3].item() == 0
    want = O.grad_norm(grads[-1].double().numpy(), 0.5)
    assert abs(clip.view(F32)[0].item() - want) <= 1e-5 * want


# ---------------------------------------------------------------- 7: the norm
NORM_N = [1, 5, 63, 64, 65, 1027, 2099201]


def _norm_bound(n):
    """Relative error bound of the reported norm against float64.

    The norm pass runs min(ceil(n / 1024), 1024) workgroups of 256 lanes; a lane takes 4 consecutive floats per trip
    and trips = ceil(n / (workgroups * 1024)) trips, adding each square to its accumulator in turn: 4 * trips fp32
    additions in a chain.  The 64 lanes of a wave then fold in 6 xor steps (6 more additions on any path), and lane 0
    adds the 4 wave sums in order (3 more).  The partials are summed and rooted in double (exact next to fp32).  So
    the longest chain of fp32 additions behind any summand is L = 4 * trips + 6 + 3.  All summands are non-negative,
    so the sum's relative error is at most L roundings plus the square's own, and the root halves it; the final
    rounding of the root to fp32 adds one: (L + 2) * 2^-24 holds.  The assertion allows twice that."""
    blocks = min(-(-n // 1024), 1024)
    trips = -(-n // (blocks * 1024))
    chain = 4 * trips + 6 + 3
    return 2.0 * (chain + 2) * 2.0 ** -24


def _measure_norm(g, gs=1.0, scaler=None, max_norm=1e30):
    """total_norm as one call of the entry reports it (the parameters it updates are scratch)."""
    n = g.numel()
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    clip, ws = torch.zeros(4, dtype=I32, device="cuda"), _ws(n)
    adamw(p, g, m, v, _adam_state(), gs=gs, scaler=scaler, max_norm=max_norm, clip=clip, ws=ws)
    return clip.view(F32)[:1].clone()


@pytest.mark.parametrize("n", NORM_N)
def test_norm(gpu, n):
    ones = torch.ones(n, device="cuda")
    got = _measure_norm(ones).item()
    want = np.float32(math.sqrt(n))
    assert abs(np.float64(got) - np.float64(want)) <= np.spacing(want), (got, want)      # 1 ulp

    gen = torch.Generator().manual_seed(77 + n)
    g = (torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 3)
         ).float()
    ref = O.grad_norm(g.double().numpy())
    gd = g.cuda()
    first = _measure_norm(gd)
    rel = abs(first.item() - ref) / ref
    print("norm n = %d: rel err %.3g, bound %.3g" % (n, rel, _norm_bound(n)))
    assert rel <= _norm_bound(n)
    assert same_bits(_measure_norm(gd), first)                                # twice on the same data: the same bits
    assert _measure_norm(gd, gs=0.5).item() == 0.5 * first.item()             # grad_scale = 0.5 halves it
    # a scaler at 1024: the norm reported is the unscaled gradient's (1024 and 1/1024 are exact factors)
    assert same_bits(_measure_norm(gd * 1024.0, scaler=_scaler(1024.0, 0)), first)


def test_misaligned_buffers_are_refused(gpu):
    """The kernels load 16 bytes at a time: an interior one float off 16-byte alignment is an error, not a fallback."""
    n = 1027
    ok = [torch.zeros(n, device="cuda") for _ in range(5)]
    off = Guarded(n, F32, torch.device("cuda"), "in", lead=1)
    for which, word in ((0, "param"), (1, "grad"), (2, "exp_avg"), (3, "exp_avg_sq"), (4, "ema")):
        a = [ctypes.c_void_p(off.data_ptr()) if k == which else ptr(t) for k, t in enumerate(ok)]
        with pytest.raises(_lib.SrkError, match=r"adamw: %s must be 16-byte aligned" % word):
            _lib.call("srk_adamw_step", a[0], a[1], a[2], a[3], n, B1, B2, EPS, ptr(_adam_state()), 1.0, None, 0.0,
                      None, 0.0, None, a[4], 0.5, None, stream_ptr())
    off.check("misaligned operand")


# ---------------------------------------------------------------- 8: the whole step
def test_whole_step_against_torch(gpu):
    """Linear(37, 5), lr 1e-2, 5 steps, weight_decay 1e-2 on the weight alone, max_norm at half the first step's
    norm, ema_decay 0.9, against CPU torch: clip_grad_norm_ + AdamW (two groups) + an EMA by hand.  1e-5 absolute is
    test_adam_matches_torch's bound at the same shape and lr."""
    torch.manual_seed(2)
    ref = torch.nn.Linear(37, 5)
    mine = torch.nn.Linear(37, 5).cuda()
    mine.load_state_dict(ref.state_dict())
    xs = [torch.randn(8, 37) for _ in range(5)]
    ref(xs[0]).pow(2).sum().backward()
    max_norm = 0.5 * float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in ref.parameters())))
    lr, wd, d = 1e-2, 1e-2, 0.9
    fp = FlatParams(mine.parameters())
    opt_m = Adam(mine.parameters(), lr=lr, flat=fp, weight_decay=wd, max_grad_norm=max_norm, ema_decay=d)
    assert opt_m.decay_mask.tolist() == [1, 1, 1, 0]
    opt_r = torch.optim.AdamW([{"params": [ref.weight], "weight_decay": wd}, {"params": [ref.bias], "weight_decay": 0.0}],
                              lr=lr)
    ema = [p.detach().clone() for p in ref.parameters()]
    clipped = 0
    for x in xs:
        opt_r.zero_grad()
        ref(x).pow(2).sum().backward()
        total = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
        clipped += total > max_norm
        opt_r.step()
        for e, p in zip(ema, ref.parameters()):
            e.mul_(d).add_(p.detach(), alpha=1 - d)
        opt_m.zero_grad()
        mine(x.cuda()).pow(2).sum().backward()
        opt_m.step()
        assert abs(opt_m.last_grad_norm() - total) <= 1e-4 * total
    assert opt_m.step_count == 5 and opt_m.clipped_steps() == clipped >= 1
    for (name, a), b, e, o in zip(ref.named_parameters(), mine.parameters(), ema, fp.offsets):
        err_p = (a.detach() - b.detach().cpu()).abs().max().item()
        err_e = (e - opt_m.ema[o:o + e.numel()].view_as(e).cpu()).abs().max().item()
        print("%s: param err %.3g, ema err %.3g" % (name, err_p, err_e))
        assert err_p <= 1e-5 and err_e <= 1e-5, name


def test_decay_reaches_marked_chunks_only(gpu):
    """Identical gradients, one step with decay and one without, n = 64 * 3 + 5 with the mask [1, 0, 1, 1] (the last
    chunk is partial): bit-equal where the chunk is not marked, different where it is."""
    n = 64 * 3 + 5
    p0, m0, v0, grads = _inputs(n, seed=3)
    g = grads[0].cuda()
    mask = torch.tensor([1, 0, 1, 1], dtype=U8, device="cuda")
    out = {}
    for wd in (0.0, 1e-2):
        p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
        adamw(p, g, m, v, _adam_state(1e-2), wd=wd, mask=mask if wd else None)
        out[wd] = (p, m, v)
    marked = torch.from_numpy(O.expand_mask(mask.cpu().numpy(), n)).cuda()
    plain, dec = out[0.0][0], out[1e-2][0]
    assert same_bits(plain[~marked], dec[~marked]) and int((~marked).sum()) == 64
    assert bool((plain[marked] != dec[marked]).all())
    assert same_bits(out[0.0][1], out[1e-2][1]) and same_bits(out[0.0][2], out[1e-2][2])     # the moments never decay
    # against the restatement, and a null mask decays every chunk
    st = O.State(p0.double().numpy())
    st.m, st.v = m0.double().numpy(), v0.double().numpy()
    O.step(st, g.cpu().double().numpy(), 1e-2, weight_decay=1e-2, mask=mask.cpu().numpy())
    assert np.abs(dec.cpu().double().numpy() - st.p).max() <= 1e-5
    p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
    adamw(p, g, m, v, _adam_state(1e-2), wd=1e-2)
    assert same_bits(p[marked], dec[marked]) and bool((p[~marked] != plain[~marked]).all())


def test_norm_pass_runs_only_where_it_is_needed(gpu):
    """One gradient read before the update with clipping on (with or without a scaler), the finite check alone with a
    scaler and no clipping, and no pass over the gradient at all with neither."""
    n = 1027
    p0, m0, v0, grads = _inputs(n, seed=1)
    g = grads[0].cuda()
    for kw, want in ((dict(wd=1e-2), (0, 0)), (dict(max_norm=1.0), (1, 0)), (dict(scaler=True), (0, 1)),
                     (dict(scaler=True, max_norm=1.0), (1, 0))):
        kw = dict(kw)
        if kw.pop("scaler", False):
            kw["scaler"] = _scaler()
        if "max_norm" in kw:
            kw.update(clip=torch.zeros(4, dtype=I32, device="cuda"), ws=_ws(n))
        p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
        try:
            _lib.prof_enable(1)
            adamw(p, g, m, v, _adam_state(), **kw)
            torch.cuda.synchronize()
            got = (_lib.prof_read("grad_norm")[0], _lib.prof_read("grad_check")[0])
            updates, _, nbytes = _lib.prof_read("adamw")
        finally:
            _lib.prof_enable(0)
        assert got == want and updates == 1, (sorted(kw), got)
        assert nbytes == (28.0 + (1.0 / 64.0 if "mask" in kw else 0.0)) * n


# ---------------------------------------------------------------- 9: the skip
def test_skipped_step_changes_nothing(gpu):
    n = 1027
    p0, m0, v0, grads = _inputs(n, seed=9)
    p, m, v, st, sc = p0.cuda(), m0.cuda(), v0.cuda(), _adam_state(), _scaler(1024.0, 0)
    ema, clip, ws = p0.cuda().clone(), torch.zeros(4, dtype=I32, device="cuda"), _ws(n)
    mask = torch.ones((n + 63) // 64, dtype=U8, device="cuda")
    kw = dict(scaler=sc, wd=1e-2, mask=mask, max_norm=0.01, clip=clip, ema=ema, d=0.9, ws=ws)
    adamw(p, grads[0].cuda() * 1024.0, m, v, st, **kw)                       # a clean, clipped step
    assert int(st[0]) == 1 and clip[2].item() == 1 and int(sc[7]) == 0
    before = [t.clone() for t in (p, m, v, ema, st)]
    bad = grads[1].cuda() * 1024.0
    bad[n - 1] = float("nan")                                               # in the scalar tail
    adamw(p, bad, m, v, st, **kw)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "ema", "state"), (p, m, v, ema, st), before):
        assert same_bits(a, b), "%s changed on a skipped step" % name
    assert clip[2].item() == 1 and int(sc[7]) == 1 and int(sc[4]) == 0      # counted; the flag cleared again
    adamw(p, grads[2].cuda() * 1024.0, m, v, st, **kw)                       # the next clean step updates
    assert int(st[0]) == 2 and clip[2].item() == 2 and int(sc[7]) == 1
    for a, b in zip((p, m, v, ema), before):
        assert not same_bits(a, b)


# ---------------------------------------------------------------- 10: guard bands and the workspace
@pytest.mark.parametrize("n", [1, 5, 1027, 2099201])
def test_guard_bands_and_workspace(gpu, n):
    """Every buffer between bands, the workspace exactly the queried size: a plain run, then guarded runs with the
    workspace pre-filled with either of WS_BYTES; the same bits every time, const inputs untouched."""
    p0, m0, v0, grads = _inputs(n, seed=5)
    nchunks = (n + 63) // 64
    mask0 = (torch.arange(nchunks) % 3 != 1).to(U8)
    ws_floats = int(_lib.lib().srk_adamw_workspace_floats(n))
    runs = []
    for guarded, ws_byte in ((False, WS_BYTES[1]), (True, WS_BYTES[0]), (True, WS_BYTES[1])):
        a = Arena(guarded, ws_byte)
        grad, mask = a.inp("grad", grads[0] * 1024.0), a.inp("decay_mask", mask0)
        p, m, v = a.out("param", n, init=p0), a.out("exp_avg", n, init=m0), a.out("exp_avg_sq", n, init=v0)
        ema = a.out("ema", n, init=p0)
        st = a.out("state", 4, I64, init=_adam_state())
        sc = a.out("scaler", 8, I32)
        clip = a.out("clip_state", 4, I32, init=torch.zeros(4, dtype=I32))
        ws = a.ws("ws", ws_floats)
        a.call("srk_grad_scaler_init", sc, 1024.0, 2.0, 0.5, 2)
        a.call("srk_adamw_step", p, grad, m, v, n, B1, B2, EPS, st, 0.5, sc, 1e-2, mask, 0.01, clip, ema, 0.9, ws)
        a.check()
        runs.append({k: b.t.clone() for k, b in (("param", p), ("exp_avg", m), ("exp_avg_sq", v), ("ema", ema),
                                                 ("state", st), ("scaler", sc), ("clip_state", clip))})
    for run in runs:
        for k, t in run.items():
            assert same_bits(t, runs[0][k]), "%s depends on the buffers around it or on the workspace's content" % k
            if t.dtype.is_floating_point:
                assert bool(torch.isfinite(t).all()), k
    assert runs[0]["clip_state"][2].item() == 1 and int(runs[0]["state"][0]) == 1
    assert not same_bits(runs[0]["param"], p0.cuda()) and not same_bits(runs[0]["ema"], p0.cuda())


# ---------------------------------------------------------------- 11: capture
@pytest.mark.parametrize("scaled", (False, True), ids=("fp32", "scaler"))
def test_captured_step_replays_the_eager_steps(gpu, scaled):
    """Linear + CrossEntropyLoss + the optimizer with clip, decay and EMA as one captured step: three replays are three
    eager steps from the same state, bit for bit."""
    from speechrecognitionproject_amd.graphs import GraphedStep
    torch.manual_seed(4)
    lin = snn.Linear(37, 5).cuda()
    fp = FlatParams(lin.parameters())
    opt = Adam(lin.parameters(), lr=1e-2, flat=fp, weight_decay=1e-2, max_grad_norm=0.05, ema_decay=0.9)
    scaler = LossScaler(1024.0, dynamic=True, growth_interval=2) if scaled else None
    crit = snn.CrossEntropyLoss()
    x, y = torch.randn(8, 37).cuda(), torch.randint(0, 5, (8,)).cuda()

    def body():
        opt.zero_grad()
        loss = crit(lin(x), y)
        (scaler.scale(loss) if scaled else loss).backward()
        opt.step(scaler=scaler)
        return loss

    bufs = [fp.data, opt.exp_avg, opt.exp_avg_sq, opt.ema, opt.clip_state, opt.state_dev]
    names = ["param", "exp_avg", "exp_avg_sq", "ema", "clip_state", "state"]
    if scaled:
        bufs.append(scaler.state)
        names.append("scaler")
    graphed = GraphedStep(body, warmup=2)
    torch.cuda.synchronize()
    start = [t.clone() for t in bufs]
    assert opt.step_count == 2                                       # the capture itself runs nothing

    replayed = []
    for _ in range(3):
        graphed.replay()
        torch.cuda.synchronize()
        replayed.append([t.clone() for t in bufs] + [graphed.out.detach().clone()])
    for t, s in zip(bufs, start):
        t.copy_(s)
    for k in range(3):
        loss = body()
        torch.cuda.synchronize()
        for name, a, b in zip(names + ["loss"], replayed[k], bufs + [loss.detach()]):
            assert same_bits(a, b), "replay %d: %s differs from the eager step" % (k, name)
    assert opt.step_count == 5 and opt.clipped_steps() >= 1
    assert not same_bits(replayed[0][0], replayed[2][0]) and not same_bits(replayed[0][3], replayed[2][3])


# ---------------------------------------------------------------- 12: ema_weights()
def test_ema_weights_swaps_contents_and_back(gpu):
    torch.manual_seed(6)
    lin = snn.Linear(37, 5).cuda()
    fp = FlatParams(lin.parameters())
    opt = Adam(lin.parameters(), lr=1e-2, flat=fp, ema_decay=0.5)
    assert same_bits(opt.ema, fp.data) and opt.ema.data_ptr() != fp.data.data_ptr()      # starts as a copy
    x = torch.randn(8, 37).cuda()
    for _ in range(3):
        opt.zero_grad()
        lin(x).pow(2).sum().backward()
        opt.step()
    assert not same_bits(opt.ema, fp.data)
    raw, avg = fp.data.clone(), opt.ema.clone()
    ptrs = [fp.data.data_ptr(), opt.ema.data_ptr()] + [p.data_ptr() for p in lin.parameters()]

    copy = snn.Linear(37, 5).cuda()                                  # a copy loaded with the EMA values
    with torch.no_grad():
        for p, o in zip(fp.params, fp.offsets):
            (copy.weight if p is lin.weight else copy.bias).copy_(avg[o:o + p.numel()].view_as(p))
        want = copy(x)
        with opt.ema_weights():
            assert same_bits(lin(x), want)
            assert same_bits(fp.data, avg) and same_bits(opt.ema, raw)
            assert ptrs == [fp.data.data_ptr(), opt.ema.data_ptr()] + [p.data_ptr() for p in lin.parameters()]
        assert same_bits(fp.data, raw) and same_bits(opt.ema, avg)   # the bits from before, both ways
        assert ptrs == [fp.data.data_ptr(), opt.ema.data_ptr()] + [p.data_ptr() for p in lin.parameters()]
        with pytest.raises(ZeroDivisionError):                       # an exception inside still swaps back
            with opt.ema_weights():
                1 / 0
        assert same_bits(fp.data, raw) and same_bits(opt.ema, avg)

    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="not inside a stream capture"):
        with torch.cuda.graph(graph):
            doubled = x * 2.0                                        # noqa: F841 — the capture is not empty
            with opt.ema_weights():
                pass
    torch.cuda.synchronize()
    assert same_bits(fp.data, raw) and same_bits(opt.ema, avg)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with Adam(lin.parameters(), lr=1e-2, flat=fp).ema_weights():
            pass


# ---------------------------------------------------------------- 13: the command line
FLAGS = ["--clip-grad-norm", "1.0", "--weight-decay", "0.01", "--ema", "0.99", "--save-model"]


def _train(tmp_path, key, extra):
    from speechrecognitionproject_amd.training import main
    # 4 steps of 16: two eager warm-ups, then the captured step replayed twice (or four eager steps)
    res = main(["-key", key, "-lr", "0.0001", "--model", "mfcc_bgru", "--synthetic", "64", "--batch-size", "16",
                "--epochs", "1", "--no-eval", "--output-path", str(tmp_path)] + extra)
    return open(tmp_path / ("loss_%s.txt" % key)).read().splitlines(), res


def test_training_cli_graph_and_eager_and_the_checkpoint(gpu, tmp_path):
    graph, res = _train(tmp_path, "g", FLAGS)
    opt, model = res["optimizer"], res["model"]
    assert opt.step_count == 4 and opt.last_grad_norm() > 0.0 and 0 <= opt.clipped_steps() <= 4
    ckpt = torch.load(tmp_path / "models" / "model_g.ckpt", map_location="cuda")
    raw_equal = True
    for name, p in model.named_parameters():
        o = opt.flat._slot[id(p)]
        assert same_bits(ckpt[name], opt.ema[o:o + p.numel()].view_as(p)), name      # the averaged weights ...
        raw_equal = raw_equal and same_bits(ckpt[name], p.detach())
    assert not raw_equal                                                             # ... not the raw ones
    eager, res_e = _train(tmp_path, "e", FLAGS + ["--no-graph"])
    assert len(graph) == 4 and np.isfinite([float(v) for v in graph]).all()
    assert graph == eager
    assert same_bits(res_e["optimizer"].ema, opt.ema) and same_bits(res_e["optimizer"].clip_state, opt.clip_state)
    plain, _ = _train(tmp_path, "p", [])
    assert len(plain) == 4 and plain[0] == graph[0] and plain[1:] != graph[1:]       # the flags change the steps


def test_training_cli_fp16(gpu, tmp_path):
    losses, res = _train(tmp_path, "h", FLAGS + ["--precision", "fp16"])
    assert len(losses) == 4 and np.isfinite([float(v) for v in losses]).all()
    assert 1 <= res["optimizer"].step_count <= 4 and (tmp_path / "models" / "model_h.ckpt").exists()
