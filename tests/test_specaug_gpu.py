"""SpecAugment on the GPU: srk_specaug_apply against the float64 restatement with explicit parameters (every edge of
the parameter domain, both layouts, both fills, both access widths, the domain limit and the per-element warp path),
invalid rows, the device draw against the Python-integer restatement, a captured draw + apply, the plugins'
``specaug=`` argument and training.py --specaug."""
import numpy as np
import pytest
import torch

import specaug_oracle as O
from tolerances import LOGITS_REL
from vtlp_oracle import uniform_f64
from speechrecognitionproject_amd import features as K
from speechrecognitionproject_amd.synthetic import synthetic_clips

pytestmark = pytest.mark.gpu

NF = NT = 2
P = O.n_params(NF, NT)
POL = {"mean": K.specaug_policy(0, NF, 0, NT, 0, fill="mean"), "zero": K.specaug_policy(0, NF, 0, NT, 0, fill="zero")}
EPS = 2.0 ** -24
INT_MAX = 2 ** 31 - 1

# (T, F): scalar path + the smallest legal warp; MFCC (scalar: 1989 elements); filter banks (16-byte path); the
# spectrogram (scalar: 15729); one clip of exactly SRK_SPECAUG_MAX_ELEMS; a long narrow clip whose frame table does
# not fit beside it in LDS (the warp computed per element)
SHAPES = {"7x5": (7, 5), "mfcc": (51, 39), "fbank": (98, 120), "spec": (49, 321), "limit": (120, 132),
          "direct": (3000, 5)}
assert SHAPES["limit"][0] * SHAPES["limit"][1] == K.SPECAUG_MAX_ELEMS
SMALL_BATCH = {"limit": (2, 5, 7), "direct": (2, 3, 5)}     # rows of explicit_rows these shapes run (B = 3)


def bits(t):
    return t.contiguous().view(torch.int32)


def explicit_rows(T, F):
    """Eight valid rows {c, w, f0, fw, f0, fw, t0, tw, t0, tw} that cover the edges of the parameter domain."""
    h = T // 2
    rows = [
        [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],                                   # c == w == 0, every width 0: the identity
        [T - 1, T - 1, 0, 1, F - 1, 1, 0, 1, T - 1, 1],                   # c == w == T-1; masks at index 0 and ending at F / T
        [T - 2, 1, 0, 2, F - 2, 2, 0, 2, T - 2, 2],                       # w = 1, the longest stretch
        [1, T - 2, F, 0, 0, 0, T, 0, 0, 0],                               # w = T-2; width 0 at the far ends
        [h, h + 1, 0, F, 1, 1, 0, 0, 0, 0],                               # a full-width frequency mask: constant clip
        [h + 1, h, 1, 3, 2, 3, 1, 3, 2, 3],                               # overlapping masks of both kinds
        [h, h, 0, 0, 0, 0, 0, T, 3, 2],                                   # a full-length time mask: constant clip
        [h - 1, h + 1, F // 2, F - F // 2, 0, 0, T // 2, T - T // 2, 0, 0],   # masks ending exactly at F and T
    ]
    rows = np.array(rows, dtype=np.int32)
    assert all(O.valid_row(r, T, F, NF, NT) for r in rows)
    return rows


class Case:
    """One shape: B clips whose means differ by 3 per clip (far above the mean fill's tolerance), their rows, the
    time-major device result for both fills and the restatement — computed once."""

    def __init__(self, name):
        self.T, self.F = T, F = SHAPES[name]
        rows = explicit_rows(T, F)
        self.rows = rows[list(SMALL_BATCH[name])] if name in SMALL_BATCH else rows
        self.B = B = len(self.rows)
        rng = np.random.default_rng(T * 1000 + F)
        self.x = (rng.standard_normal((B, T, F)) + 3.0 * np.arange(B)[:, None, None] - 5.0).astype(np.float32)
        self.xd = torch.from_numpy(self.x).cuda()
        self.pd = torch.from_numpy(self.rows).cuda()
        self.out = {fill: K.spec_augment(self.xd, self.pd, POL[fill]) for fill in POL}
        self.ref = {fill: O.apply(self.x, self.rows, NF, NT, fill) for fill in POL}


_cases = {}


@pytest.fixture(params=list(SHAPES))
def case(request, gpu):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def check_against_oracle(x, out, ref, fill, tag=""):
    """The three element classes of the issue: copies bit-equal, warped within 8 ulp-of-the-operands, masked all
    one value (0 exactly, or the float64 mean within the worst case of any fp32 summation order)."""
    y, mask, ii, aa, fills = ref
    B, T, F = x.shape
    n_copy = n_warp = n_mask = 0
    for b in range(B):
        i, a = ii[b], aa[b]
        x0 = x[b][i]
        x1 = x[b][np.minimum(i + 1, T - 1)]
        copy = (~mask[b]) & (a[:, None] == 0)
        warp = (~mask[b]) & (a[:, None] != 0)
        assert out[b][copy].tobytes() == x0[copy].tobytes(), (tag, b, "copied elements are not bit-equal")
        bound = 8 * EPS * (np.abs(x0).astype(np.float64) + np.abs(x1))
        err = np.abs(out[b].astype(np.float64) - y[b])
        if warp.any():
            worst = float((err[warp] / bound[warp]).max())
            print("%s clip %d: %d warped elements, worst error / bound %.3f" % (tag, b, int(warp.sum()), worst))
            assert (err[warp] <= bound[warp]).all(), (tag, b, worst)
        if mask[b].any():
            vals = np.unique(out[b][mask[b]].view(np.int32))
            assert len(vals) == 1, (tag, b, "masked elements differ")
            v = float(vals.view(np.float32)[0])
            if fill == "zero":
                assert vals[0] == 0, (tag, b, v)                     # +0.0 exactly
            else:
                tol = T * F * EPS * float(np.abs(x[b].astype(np.float64)).mean())
                print("%s clip %d: mean fill %.7g vs %.7g (tolerance %.3g)" % (tag, b, v, fills[b], tol))
                assert abs(v - fills[b]) <= tol, (tag, b, v, fills[b], tol)
        n_copy, n_warp, n_mask = n_copy + int(copy.sum()), n_warp + int(warp.sum()), n_mask + int(mask[b].sum())
    return n_copy, n_warp, n_mask


@pytest.mark.parametrize("fill", ["mean", "zero"])
def test_apply_against_the_restatement(case, fill):
    out = case.out[fill].cpu().numpy()
    n_copy, n_warp, n_mask = check_against_oracle(case.x, out, case.ref[fill], fill, "%dx%d" % (case.T, case.F))
    assert n_copy > 0 and n_warp > 0 and n_mask > 0
    mask = case.ref[fill][1]
    full = [b for b in range(case.B) if mask[b].all()]
    assert full or case.B == 3                                   # rows 4 and 6 are fully masked clips
    for b in full:
        assert len(np.unique(out[b].view(np.int32))) == 1
    # c == w: every unmasked frame is a bit-exact copy of itself
    for b in range(case.B):
        if case.rows[b][0] == case.rows[b][1]:
            keep = ~mask[b]
            assert out[b][keep].tobytes() == case.x[b][keep].tobytes()


@pytest.mark.parametrize("fill", ["mean", "zero"])
def test_freq_major_is_the_transpose_bit_for_bit(case, fill):
    xt = case.xd.transpose(1, 2).contiguous()                       # [B, F, T]
    ft = K.spec_augment(xt, case.pd, POL[fill], time_major=False)
    assert ft.shape == (case.B, case.F, case.T)
    assert torch.equal(bits(ft), bits(case.out[fill].transpose(1, 2)))
    inplace = xt.clone()
    assert K.spec_augment(inplace, case.pd, POL[fill], time_major=False, out=inplace) is inplace
    assert torch.equal(bits(inplace), bits(ft))


@pytest.mark.parametrize("fill", ["mean", "zero"])
def test_in_place_equals_out_of_place(case, fill):
    buf = case.xd.clone()
    got = K.spec_augment(buf, case.pd, POL[fill], out=buf)
    assert got is buf and torch.equal(bits(buf), bits(case.out[fill]))


def test_rows_do_not_depend_on_the_batch(case):
    for n in (1, 3, case.B):
        got = K.spec_augment(case.xd[:n], case.pd[:n], POL["mean"])
        assert torch.equal(bits(got), bits(case.out["mean"][:n]))
    # a batch that starts at clip 1: when T F is odd its clips sit at other alignments
    got = K.spec_augment(case.xd[1:], case.pd[1:], POL["mean"])
    assert torch.equal(bits(got), bits(case.out["mean"][1:]))


def test_each_clip_uses_its_own_row(case):
    same = case.xd[:1].repeat(case.B, 1, 1)
    batch = K.spec_augment(same, case.pd, POL["mean"])
    single = torch.cat([K.spec_augment(same[:1], case.pd[b:b + 1], POL["mean"]) for b in range(case.B)])
    assert torch.equal(bits(batch), bits(single))
    assert not torch.equal(bits(batch[0]), bits(batch[1]))


def invalid_rows(T, F):
    good = [T // 2, T // 2 + 1, 1, 2, 0, 0, 1, 2, 0, 0]

    def with_(**kw):
        r = list(good)
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r
    return {
        "c=0,w=1": with_(_0=0, _1=1), "w=T-1": with_(_1=T - 1), "c=T-1": with_(_0=T - 1), "c<0": with_(_0=-1, _1=-1),
        "c=w=T": with_(_0=T, _1=T), "w=0": with_(_1=0), "c huge": with_(_0=INT_MAX), "w most negative": with_(_1=-INT_MAX - 1),
        "f0<0": with_(_2=-1), "fw<0": with_(_3=-1), "f0+fw>F": with_(_2=F - 1, _3=2), "f0>F": with_(_4=F + 1, _5=0),
        "fw overflows": with_(_2=2, _3=INT_MAX), "second f mask": with_(_4=0, _5=F + 1),
        "t0<0": with_(_6=-2), "tw<0": with_(_7=-1), "t0+tw>T": with_(_6=T - 1, _7=2), "tw overflows": with_(_8=1, _9=INT_MAX),
        "t0 huge": with_(_8=INT_MAX, _9=INT_MAX),
    }


@pytest.mark.parametrize("name", ["7x5", "fbank"])
@pytest.mark.parametrize("time_major", [True, False], ids=["tf", "ft"])
def test_invalid_rows_give_nan_clips_and_leave_the_neighbours(gpu, name, time_major):
    T, F = SHAPES[name]
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((3, T, F)).astype(np.float32)).cuda()
    if not time_major:
        x = x.transpose(1, 2).contiguous()
    good = invalid_rows(T, F)["c=0,w=1"]
    good[0] = T // 2
    assert O.valid_row(good, T, F, NF, NT)
    clean = K.spec_augment(x, [good] * 3, POL["mean"], time_major=time_major)
    assert bool(torch.isfinite(clean).all())
    for kind, row in invalid_rows(T, F).items():
        assert not O.valid_row(row, T, F, NF, NT), kind
        out = K.spec_augment(x, [good, row, good], POL["mean"], time_major=time_major)
        assert bool(torch.isnan(out[1]).all()), kind
        assert torch.equal(bits(out[0]), bits(clean[0])) and torch.equal(bits(out[2]), bits(clean[2])), kind
    # the process goes on
    again = K.spec_augment(x, [good] * 3, POL["mean"], time_major=time_major)
    assert torch.equal(bits(again), bits(clean))


def test_wrapper_argument_checks(gpu):
    x = torch.zeros(2, 7, 5, device="cuda")
    rows = [[0] * P] * 2
    with pytest.raises(K.SrkError):
        K.spec_augment(x, [[0] * P] * 3, POL["mean"])                     # one row too many
    with pytest.raises(K.SrkError):
        K.spec_augment(x, torch.zeros(2, P, dtype=torch.int64), POL["mean"])
    with pytest.raises(K.SrkError):
        K.spec_augment(x.double(), rows, POL["mean"])
    with pytest.raises(K.SrkError):
        K.spec_augment(x.transpose(1, 2), rows, POL["mean"])              # not contiguous
    with pytest.raises(K.SrkError, match="specaug"):
        K.spec_augment(torch.zeros(1, 120, 133, device="cuda"), [[0] * P], POL["mean"])   # above the domain
    with pytest.raises(K.SrkError, match="specaug"):
        K.specaug_draw(4, 6, 5, (2, 0, 0, 0, 0))                          # W = 2 needs 7 frames
    assert K.spec_augment(torch.zeros(0, 7, 5, device="cuda"), torch.zeros(0, P, dtype=torch.int32), POL["mean"]).shape == (0, 7, 5)


DRAWN = (("fbank", (5, 2, 15, 2, 12)), ("mfcc", (3, 2, 6, 2, 8)), ("spec", (4, 2, 40, 2, 8)))


@pytest.mark.parametrize("name,policy", DRAWN, ids=[d[0] for d in DRAWN])
def test_draws_equal_the_restatement_and_apply_with_them(gpu, name, policy):
    T, F = SHAPES[name]
    pol = K.specaug_policy(*policy)
    rng = np.random.default_rng(F)
    x = (rng.standard_normal((24, T, F)) * 4.0 + 2.0 * np.arange(24)[:, None, None] - 20.0).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    K.specaug_reseed(1234)
    assert K.specaug_state() == (1234, 0)
    for counter in (0, 1):
        pd = K.specaug_draw(24, T, F, pol)
        assert K.specaug_state() == (1234, counter + 1)
        p = pd.cpu().numpy()
        want = O.draw(1234, counter, 24, T, F, *policy)
        assert p.dtype == np.int32 and p.tobytes() == want.tobytes()
        shares = [O.masked_share(r, T, F, NF, NT) for r in p]
        warped = int((p[:, 0] != p[:, 1]).sum())
        print("%s counter %d: masked share %.3f .. %.3f, %d of 24 clips warped" % (name, counter, min(shares), max(shares), warped))
        assert 0.05 <= min(shares) and max(shares) <= 0.5
        assert warped >= 20
        for time_major in (True, False):
            src = xd if time_major else xd.transpose(1, 2).contiguous()
            out = K.spec_augment(src, pd, pol, time_major=time_major)
            out = out if time_major else out.transpose(1, 2)
            _, n_warp, n_mask = check_against_oracle(x, out.cpu().numpy(), O.apply(x, p, NF, NT, "mean"), "mean",
                                                     "%s k=%d %s" % (name, counter, "tf" if time_major else "ft"))
            assert n_warp > 0 and n_mask > 0


def test_draw_shapes_and_the_smallest_warp(gpu):
    K.specaug_reseed(7)
    p = K.specaug_draw(256, 7, 5, (2, 1, 5, 1, 7)).cpu().numpy()           # T = 2W + 3
    assert p.tobytes() == O.draw(7, 0, 256, 7, 5, 2, 1, 5, 1, 7).tobytes()
    assert (p[:, 0] == 3).all() and set(p[:, 1].tolist()) == {1, 2, 3, 4, 5}
    assert all(O.valid_row(r, 7, 5, 1, 1) for r in p)
    q = K.specaug_draw(3, 98, 120, (0, 4, 120, 4, 98)).cpu().numpy()       # no warp, the most masks, the widest bounds
    assert q.shape == (3, 18) and q.tobytes() == O.draw(7, 1, 3, 98, 120, 0, 4, 120, 4, 98).tobytes()
    r = K.specaug_draw(5, 98, 120, K.specaug_policy(5, 2, 15, 2, 60, p=0.1)).cpu().numpy()   # t_max = floor(0.1 * 98)
    assert r.tobytes() == O.draw(7, 2, 5, 98, 120, 5, 2, 15, 2, 9).tobytes()
    out = torch.empty(1000, 2, dtype=torch.int32, device="cuda")           # more clips than the draw's workgroup
    assert K.specaug_draw(1000, 51, 39, (3, 0, 0, 0, 0), out=out) is out
    assert out.cpu().numpy().tobytes() == O.draw(7, 3, 1000, 51, 39, 3, 0, 0, 0, 0).tobytes()
    assert K.specaug_state() == (7, 4)


def test_captured_draw_and_apply_replay(gpu):
    """specaug_draw into a static buffer, then spec_augment in place on a static copy of the features, captured as
    one chain: every replay draws the next counter's rows (the kernel advances the counter) and applies them."""
    from speechrecognitionproject_amd.graphs import GraphedStep
    T, F = SHAPES["fbank"]
    pol = K.specaug_policy(5, 2, 15, 2, 12)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((4, T, F)).astype(np.float32)).cuda()
    buf = torch.empty(4, pol.n_params, dtype=torch.int32, device="cuda")
    feat = torch.empty_like(x)
    K.specaug_reseed(99)

    def body():
        feat.copy_(x)
        K.specaug_draw(4, T, F, pol, out=buf)
        return K.spec_augment(feat, buf, pol, out=feat)

    g = GraphedStep(body, warmup=2)
    base, counter = K.specaug_state()
    assert (base, counter) == (99, 2)            # two warm-up calls; the capture itself draws nothing
    for k in (counter, counter + 1):
        out = g.replay()
        torch.cuda.synchronize()
        want = O.draw(base, k, 4, T, F, 5, 2, 15, 2, 12)
        assert buf.cpu().numpy().tobytes() == want.tobytes()
        eager = K.spec_augment(x, torch.from_numpy(want).cuda(), pol)
        assert torch.equal(bits(out), bits(eager))
    assert K.specaug_state() == (99, counter + 2)
    g.release()


# ---------------------------------------------------------------- the plugins
MODELS = {
    "mfcc_bgru": ("model_mfcc_bgru", {}, (51, 39), (3, 2, 6, 2, 8)),
    "mfcc_bgru_40x98": ("model_mfcc_bgru", {"features": "mfcc40x98"}, (98, 40), (5, 2, 8, 2, 12)),
    "mfcc_bgru_att": ("model_mfcc_bgru_att", {}, (51, 39), (3, 2, 6, 2, 8)),
    "spec_bgru": ("model_spec_bgru", {}, (49, 321), (4, 2, 40, 2, 8)),
    "spec_cnn": ("model_spec_cnn", {}, (49, 321), (4, 2, 40, 2, 8)),
    "fbanks_cnn": ("model_fbanks_cnn", {}, (98, 120), (5, 2, 15, 2, 12)),
    "fbanks_cnn_pcen": ("model_fbanks_cnn_pcen", {}, (98, 120), (5, 2, 15, 2, 12)),
    "fbanks_dscnn": ("model_fbanks_dscnn", {}, (98, 120), (5, 2, 15, 2, 12)),
}


@pytest.fixture(scope="module")
def clips(gpu):
    x, _ = synthetic_clips(4, seed=21)
    return torch.from_numpy(x).cuda()


@pytest.mark.parametrize("name", list(MODELS))
def test_plugin_with_specaug(clips, name):
    import importlib
    module, kwargs, (T, F), policy = MODELS[name]
    M = importlib.import_module("speechrecognitionproject_amd.models." + module)
    torch.manual_seed(3)
    plain = M.Network(**kwargs).cuda()
    aug = M.Network(specaug=policy, **kwargs).cuda()
    aug.load_state_dict(plain.state_dict())
    for net in (plain, aug):
        if hasattr(net, "dropout"):
            net.dropout.p = 0.0                      # the comparison is about the features, not the masks
    pol = K.specaug_policy(*policy)
    assert aug.specaug == pol and plain.specaug is None

    # eval() never augments
    plain.eval(), aug.eval()
    K.specaug_reseed(5)
    with torch.no_grad():
        assert torch.equal(bits(aug(clips)), bits(plain(clips)))
    assert K.specaug_state() == (5, 0) and aug.last_specaug is None

    # train mode, all-identity rows: the plain model bit for bit (BatchNorm statistics included)
    plain.train(), aug.train()
    identity = torch.zeros(4, pol.n_params, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        ref = plain(clips)
        same = aug(clips, specaug_params=identity)
    assert torch.equal(bits(same), bits(ref))
    assert aug.last_specaug is identity and K.specaug_state() == (5, 0)

    # drawn rows: the restatement's, and the logits move
    out = aug(clips)
    drawn = aug.last_specaug
    assert drawn.dtype == torch.int32 and tuple(drawn.shape) == (4, pol.n_params)
    assert drawn.cpu().numpy().tobytes() == O.draw(5, 0, 4, T, F, *policy).tobytes()
    moved = float((out.detach() - ref).abs().max() / ref.abs().max())
    print("%s: logits moved by %.3g of their scale" % (name, moved))
    assert moved > 100 * LOGITS_REL
    aug(clips)
    assert aug.last_specaug is drawn and K.specaug_state() == (5, 2)       # one persistent buffer per batch size
    assert drawn.cpu().numpy().tobytes() == O.draw(5, 1, 4, T, F, *policy).tobytes()

    # backward
    aug.zero_grad()
    out.sum().backward()
    grads = {k: p.grad for k, p in aug.named_parameters() if p.requires_grad}
    # spec_cnn keeps the reference's bn1, which no forward calls (models/model_spec_cnn.py): it alone gets no gradient
    unused = ["bn1.weight", "bn1.bias"] if name == "spec_cnn" else []
    assert sorted(k for k, g in grads.items() if g is None) == sorted(unused)
    grads = [g for g in grads.values() if g is not None]
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool((g != 0).any()) for g in grads)

    with pytest.raises(ValueError):
        plain(clips, specaug_params=identity)                                # no policy to read the rows with


def test_fbanks_cnn_with_vtlp_and_specaug(clips):
    from speechrecognitionproject_amd.models import model_fbanks_cnn as M
    torch.manual_seed(3)
    net = M.Network(vtlp=(0.9, 1.1), specaug=(5, 2, 15, 2, 12)).cuda().train()
    net.dropout.p = 0.0
    K.specaug_reseed(8)
    K.vtlp_reseed(8)
    with torch.no_grad():
        out = net(clips)
        alpha, rows = net.last_alpha.clone(), net.last_specaug.clone()
        assert K.vtlp_state() == (8, 1) and K.specaug_state() == (8, 1)
        assert alpha.cpu().numpy().tobytes() == uniform_f64(8, 0, 4, 0.9, 1.1).tobytes()
        assert rows.cpu().numpy().tobytes() == O.draw(8, 0, 4, 98, 120, 5, 2, 15, 2, 12).tobytes()
        # the bank is warped first, then masked: the same draws given explicitly are the same forward
        again = net(clips, alpha=alpha, specaug_params=rows)
        warped_only = net(clips, alpha=alpha, specaug_params=torch.zeros(4, 10, dtype=torch.int32))
    assert bool(torch.isfinite(out).all())
    assert torch.equal(bits(again), bits(out))
    assert not torch.equal(out, warped_only)
    assert K.vtlp_state() == (8, 1) and K.specaug_state() == (8, 1)


# ---------------------------------------------------------------- training.py
def _train(tmp_path, key, model, specaug, extra):
    from speechrecognitionproject_amd.training import main
    K.specaug_reseed(77)
    # 4 steps of 8: two eager warm-ups, then the captured step replayed twice (or four eager steps)
    main(["-key", key, "-lr", "0.0001", "--model", model, "--specaug", specaug, "--synthetic", "16", "--batch-size", "8",
          "--epochs", "2", "--no-eval", "--output-path", str(tmp_path)] + extra)
    return open(tmp_path / ("loss_%s.txt" % key)).read().splitlines()


def test_training_cli_graph_and_eager_write_the_same_losses(gpu, tmp_path):
    """mfcc_bgru has no dropout and the draw's counter lives on the device: the replayed steps are the eager ones."""
    graph = _train(tmp_path, "g", "mfcc_bgru", "3,2,6,2,8", [])
    eager = _train(tmp_path, "e", "mfcc_bgru", "3,2,6,2,8", ["--no-graph"])
    assert len(graph) == 4 and np.isfinite([float(v) for v in graph]).all()
    assert graph == eager
    assert K.specaug_state() == (77, 4)


def test_training_cli_fbanks_cnn(gpu, tmp_path):
    losses = _train(tmp_path, "f", "fbanks_cnn", "5,2,15,2,12", ["--specaug-fill", "zero"])
    assert len(losses) == 4 and np.isfinite([float(v) for v in losses]).all()


def test_training_cli_rejects_specaug_for_other_models(gpu):
    from speechrecognitionproject_amd.training import main
    with pytest.raises(SystemExit):
        main(["--model", "resnet_bgru", "--specaug", "3,2,6,2,8", "--synthetic", "16", "--batch-size", "8", "--no-eval"])
