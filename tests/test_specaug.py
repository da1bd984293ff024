"""SpecAugment without a GPU: the restatement of the device draw stays in its domain, both entry points validate on
the host before any device work, the policy helper and the training CLI accept and reject as specified."""
import ctypes

import numpy as np
import pytest

import specaug_oracle as O
from speechrecognitionproject_amd import _lib
from speechrecognitionproject_amd import features as K

PTR = ctypes.c_void_p(256)      # a non-null, 16-byte aligned "device pointer": validation never dereferences it
I64 = ctypes.c_int64
MAX = K.SPECAUG_MAX_ELEMS

# the three model feature shapes with the policies of the GPU tests
POLICIES = (((98, 120), (5, 2, 15, 2, 12)), ((51, 39), (3, 2, 6, 2, 8)), ((49, 321), (4, 2, 40, 2, 8)))


def test_header_constant_matches_python():
    text = open(_lib.HEADER).read()
    assert "#define SRK_SPECAUG_MAX_ELEMS %d" % MAX in text
    assert MAX >= 15729                                   # 49 x 321, the largest of the four feature shapes
    for T, F in ((51, 39), (98, 40), (98, 120), (49, 321)):
        assert T * F <= MAX


def test_abi_declares_and_binds_both_symbols():
    syms = _lib.header_symbols()
    L = _lib.lib()
    for s in ("srk_specaug_apply", "srk_specaug_draw"):
        assert s in syms and s in _lib._SIGS and hasattr(L, s)


def test_draw_restatement_stays_in_its_domain():
    shapes = [(7, 5, 2), (5, 3, 1), (9, 4, 3), (51, 39, 3), (51, 39, 24), (98, 120, 5), (98, 40, 47), (49, 321, 4),
              (49, 321, 23), (1, 1, 0), (2, 7, 0), (120, 132, 58)]
    n = 0
    for T, F, W in shapes:
        assert W == 0 or T >= 2 * W + 3
        for seed in range(12):
            NF, NT = seed % 5, (seed // 2) % 5
            f_max, t_max = (F, T) if seed % 3 == 0 else (F // 2, T // 3)
            p = O.draw(0x1234567 * (seed + 1), seed, 16, T, F, W, NF, f_max, NT, t_max)
            assert p.shape == (16, O.n_params(NF, NT)) and p.dtype == np.int32
            for row in p:
                assert O.valid_row(row, T, F, NF, NT), (T, F, W, row)
                c, w = int(row[0]), int(row[1])
                if W == 0:
                    assert c == 0 and w == 0
                else:
                    assert W + 1 <= c <= T - W - 2 and abs(w - c) <= W
                assert all(0 <= int(row[3 + 2 * j]) <= f_max for j in range(NF))
                assert all(0 <= int(row[3 + 2 * NF + 2 * j]) <= t_max for j in range(NT))
                n += 1
    assert n == len(shapes) * 12 * 16
    # T = 2W + 3: the one legal centre, every shift of it
    p = O.draw(99, 0, 256, 7, 5, 2, 0, 0, 0, 0)
    assert (p[:, 0] == 3).all() and set(p[:, 1].tolist()) == {1, 2, 3, 4, 5}


def test_draw_restatement_depends_on_counter_and_clip():
    a = O.draw(1234, 0, 8, 98, 120, 5, 2, 15, 2, 12)
    assert not np.array_equal(a, O.draw(1234, 1, 8, 98, 120, 5, 2, 15, 2, 12))
    assert np.array_equal(a[:3], O.draw(1234, 0, 3, 98, 120, 5, 2, 15, 2, 12))    # a row depends on its index only
    assert len({tuple(r) for r in a.tolist()}) == 8


@pytest.mark.parametrize("shape_policy", POLICIES, ids=lambda sp: "%dx%d" % sp[0])
def test_masked_share_and_warped_clips_of_the_restatement(shape_policy):
    """What keeps the GPU comparison on drawn parameters from being vacuous (tests/test_specaug_gpu.py)."""
    (T, F), pol = shape_policy
    for counter in (0, 1):
        p = O.draw(1234, counter, 24, T, F, *pol)
        shares = [O.masked_share(r, T, F, pol[1], pol[3]) for r in p]
        assert 0.05 <= min(shares) and max(shares) <= 0.5, (min(shares), max(shares))
        assert int((p[:, 0] != p[:, 1]).sum()) >= 20


def test_apply_restatement_basics():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 7, 5)).astype(np.float32)
    rows = np.array([[0, 0, 0, 0, 0, 0], [3, 1, 1, 2, 5, 2], [9, 1, 0, 0, 0, 0]], dtype=np.int32)
    y, mask, i, a, fills = O.apply(x, rows, 1, 1, "mean")
    assert np.array_equal(y[0], x[0].astype(np.float64)) and not mask[0].any()
    assert np.isnan(y[2]).all()                                        # c = 9 is outside a 7-frame clip
    # c = 3 -> w = 1: s = 3t for t <= 1, then 3 + (t - 1) * 3 / 5
    assert i[1].tolist() == [0, 3, 3, 4, 4, 5, 6] and np.allclose(a[1], [0, 0, .6, .2, .8, .4, 0])
    assert mask[1][:, 1:3].all() and mask[1][5:7].all() and not mask[1][:5, [0, 3, 4]].any()
    assert (y[1][mask[1]] == fills[1]).all() and fills[1] == x[1].astype(np.float64).mean()
    assert y[1][2, 0] == x[1][3, 0] + 0.6 * (np.float64(x[1][4, 0]) - x[1][3, 0])


def _apply(x=PTR, B=2, T=98, F=120, tm=1, params=PTR, NF=2, NT=2, mode=1, value=0.0, y=PTR):
    L = _lib.lib()
    rc = L.srk_specaug_apply(x, B, T, F, tm, params, NF, NT, mode, value, y, None)
    return rc, L.srk_last_error()


@pytest.mark.parametrize("kw", [
    dict(T=120, F=133), dict(T=1, F=MAX + 1), dict(T=MAX + 1, F=1), dict(T=1 << 20, F=1 << 20), dict(B=0), dict(B=-3),
    dict(T=0), dict(F=0), dict(T=-1), dict(NF=5), dict(NF=-1), dict(NT=5), dict(NT=-1), dict(mode=2), dict(mode=-1),
    dict(value=float("nan")), dict(value=float("inf")), dict(value=float("-inf"), mode=0), dict(x=None),
    dict(params=None), dict(y=None), dict(tm=2)], ids=str)
def test_apply_refuses_invalid_arguments(kw):
    rc, err = _apply(**kw)
    assert rc == -1 and b"specaug" in err, (rc, err)


def _draw(state=PTR, B=4, T=98, F=120, W=5, NF=2, f_max=15, NT=2, t_max=12, out=PTR):
    L = _lib.lib()
    rc = L.srk_specaug_draw(state, B, T, F, W, NF, f_max, NT, t_max, out, None)
    return rc, L.srk_last_error()


@pytest.mark.parametrize("kw", [
    dict(W=-1), dict(W=48), dict(T=6, W=2, t_max=0), dict(T=2, W=1, t_max=0), dict(f_max=121), dict(f_max=-1),
    dict(t_max=99), dict(t_max=-1), dict(B=0), dict(T=0, W=0, t_max=0), dict(F=0, f_max=0), dict(NF=5), dict(NT=-1),
    dict(state=None), dict(out=None)], ids=str)
def test_draw_refuses_invalid_arguments(kw):
    rc, err = _draw(**kw)
    assert rc == -1 and b"specaug" in err, (rc, err)


def test_policy_helper():
    p = K.specaug_policy(5, 2, 15, 2, 12)
    assert tuple(p) == (5, 2, 15, 2, 12, 1.0, "mean") and p.n_params == 10
    assert K.specaug_policy(0, 0, 0, 0, 0, fill="zero").n_params == 2
    assert K.as_specaug_policy((3, 2, 6, 2, 8)) == K.specaug_policy(3, 2, 6, 2, 8)
    assert K.as_specaug_policy(p) is p
    # the effective time-mask bound: min(t_max, floor(p T)), applied where T is known
    q = K.specaug_policy(5, 2, 15, 2, 40, p=0.2)
    assert q.t_max_for(98) == 19 and q.t_max_for(51) == 10 and q.t_max_for(400) == 40 and p.t_max_for(98) == 12
    for bad in ((-1, 2, 15, 2, 12), (5, 5, 15, 2, 12), (5, 2, 15, 5, 12), (5, 2, -1, 2, 12), (5, 2, 15, 2, -2),
                (5.5, 2, 15, 2, 12), (5, 2, 15, 2, 12, 1.5), (5, 2, 15, 2, 12, -0.1), (5, 2, 15, 2, 12, 1.0, "median"),
                (True, 2, 15, 2, 12)):
        with pytest.raises(ValueError):
            K.specaug_policy(*bad)
    assert p.check_shape(98, 120) is p and p.check_shape(13, 15) is p
    for T, F in ((12, 120), (98, 14), (11, 120), (200, 120)):       # W, f_max, t_max, the domain
        with pytest.raises(ValueError):
            p.check_shape(T, F)


def test_plugins_take_and_check_the_argument():
    from speechrecognitionproject_amd.models import model_mfcc_bgru as M
    from speechrecognitionproject_amd.training import SPECAUG_SHAPES
    assert sorted(SPECAUG_SHAPES) == ["fbanks_cnn", "fbanks_cnn_pcen", "fbanks_dscnn", "mfcc_bgru", "mfcc_bgru_att",
                                      "spec_bgru", "spec_cnn"]
    net = M.Network(num_features=128, specaug=(3, 2, 6, 2, 8))
    assert net.specaug == K.specaug_policy(3, 2, 6, 2, 8) and net.last_specaug is None
    assert M.Network(num_features=128).specaug is None
    assert not [k for k in net.state_dict() if "specaug" in k]     # checkpoints are unchanged
    with pytest.raises(ValueError):
        M.Network(num_features=128, specaug=(3, 2, 40, 2, 8))      # f_max above the 39 features
    with pytest.raises(ValueError):
        M.Network(num_features=128, specaug=(25, 2, 6, 2, 8))      # W = 25 needs 53 frames
    assert M.Network(num_features=128, features="mfcc40x98", specaug=(25, 2, 40, 2, 8)).specaug.W == 25


def test_training_cli_specaug_flags():
    from speechrecognitionproject_amd.training import parse
    assert parse(["--model", "mfcc_bgru"]).specaug is None
    a = parse(["--model", "mfcc_bgru", "--specaug", "3,2,6,2,8"])
    assert a.specaug == K.specaug_policy(3, 2, 6, 2, 8) and a.specaug.fill == "mean"
    a = parse(["--model", "fbanks_cnn", "--specaug", "5,2,15,2,12", "--specaug-fill", "zero", "--vtlp", "0.9,1.1"])
    assert a.specaug == K.specaug_policy(5, 2, 15, 2, 12, fill="zero") and a.vtlp == (0.9, 1.1)
    assert parse(["--model", "spec_cnn", "--specaug", "4,2,40,2,8"]).specaug.f_max == 40
    assert parse(["--specaug", "0,0,0,0,0"]).specaug.n_params == 2            # the default model is mfcc_bgru
    for argv in (["--model", "resnet_bgru", "--specaug", "3,2,6,2,8"],         # no such argument on the plugin
                 ["--model", "cnn_bgru", "--specaug", "3,2,6,2,8"],
                 ["--model", "mfcc_bgru", "--specaug", "3,2,6,2"],              # four values
                 ["--model", "mfcc_bgru", "--specaug", "3,2,6,2,8,1"],
                 ["--model", "mfcc_bgru", "--specaug", "3,2,x,2,8"],
                 ["--model", "mfcc_bgru", "--specaug", "3,2,6.5,2,8"],
                 ["--model", "mfcc_bgru", "--specaug", "3,2,40,2,8"],           # f_max above 39 features
                 ["--model", "mfcc_bgru", "--specaug", "25,2,6,2,8"],           # W against 51 frames
                 ["--model", "mfcc_bgru", "--specaug", "3,2,6,2,52"],           # t_max above 51 frames
                 ["--model", "mfcc_bgru", "--specaug", "3,5,6,2,8"],            # five masks
                 ["--model", "mfcc_bgru", "--specaug", "-1,2,6,2,8"],
                 ["--model", "mfcc_bgru", "--specaug", "3,2,6,2,8", "--specaug-fill", "median"]):
        with pytest.raises(SystemExit):
            parse(argv)
