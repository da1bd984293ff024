"""The transformer-encoder pieces and the fbanks_kwt plugin without a GPU: the hand-written backward formulas of
tests/kwt_oracle.py against float64 autograd (torch's own encoder layer included), the modules' parameters against
torch's, the CLI choice, the state_dict layouts, and the host-side argument checks of srk_mhsa_*, srk_layernorm_* and
srk_gelu_*."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import kwt_oracle as KO


def _rel(got, want):
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-300))


# ----------------------------------------------------------------------------- the oracle's own formulas
@pytest.mark.parametrize("case", [(2, 3, 7, 8, 1), (2, 2, 1, 4, 1), (2, 2, 65, 20, 1), (1, 1, 33, 16, 3)])
def test_attention_formulas_equal_float64_autograd(case):
    c = KO.attn_case(*case)
    B, H, T, dh, _ = case
    qkv = c["qkv"].clone().requires_grad_(True)
    q, k, v = (t.reshape(B, T, H, dh).transpose(1, 2) for t in qkv.split(H * dh, dim=2))
    # torch's scaled_dot_product_attention uses the same default scale, dh ** -0.5
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, H * dh)
    (o * c["do"]).sum().backward()
    assert _rel(c["o"], o.detach()) <= 1e-12
    assert _rel(c["dqkv"], qkv.grad) <= 1e-12
    s = c["scale"] * (q.detach() @ k.detach().transpose(2, 3))
    assert _rel(c["lse"], torch.logsumexp(s, dim=3)) <= 1e-12


@pytest.mark.parametrize("shape", [(5, 64), (3, 130), (1, 1), (7, 3)])
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_formulas_equal_float64_autograd(shape, with_res):
    c = KO.ln_case(*shape, with_res, 0)
    x = c["x"].clone().requires_grad_(True)
    gamma, beta = c["gamma"].clone().requires_grad_(True), c["beta"].clone().requires_grad_(True)
    s = x if c["res"] is None else x + c["res"]
    y = F.layer_norm(s, (shape[1],), gamma, beta, KO.LN_EPS)
    (y * c["dy"]).sum().backward()
    assert _rel(c["y"], y.detach()) <= 1e-12
    if shape[1] > 1:      # D = 1: y == beta and ds == 0 exactly on both sides
        assert _rel(c["ds"], x.grad) <= 1e-12
        assert _rel(c["dgamma"], gamma.grad) <= 1e-12
    else:
        assert float(c["ds"].abs().max()) == 0.0 and torch.equal(c["y"], c["beta"].expand_as(c["y"]))
    assert _rel(c["dbeta"], beta.grad) <= 1e-12


def test_gelu_formulas_equal_float64_autograd():
    x = torch.linspace(-12, 12, 4801, dtype=torch.float64).requires_grad_(True)
    dy = torch.cos(torch.arange(4801, dtype=torch.float64))
    y = F.gelu(x)
    (y * dy).sum().backward()
    assert _rel(KO.gelu(x.detach()), y.detach()) <= 1e-12
    assert _rel(KO.gelu_backward(x.detach(), dy), x.grad) <= 1e-12


@pytest.mark.parametrize("dims", [(64, 1, 256), (24, 3, 20)])
def test_formulas_compose_to_torchs_encoder_layer(dims):
    """torch.nn.TransformerEncoderLayer in float64, training mode, equals the spelled-out formulas with the in_proj
    column order the kernels read: the layer is an independent oracle for layout and arithmetic alike."""
    d, h, ff = dims
    torch.manual_seed(4)
    layer = torch.nn.TransformerEncoderLayer(d, h, ff, dropout=0.0, activation="gelu", batch_first=True).double().train()
    x = torch.randn(2, 7, d, dtype=torch.float64)
    sd = layer.state_dict()
    qkv = x @ sd["self_attn.in_proj_weight"].T + sd["self_attn.in_proj_bias"]
    o, _ = KO.mhsa(qkv, h, (d // h) ** -0.5)
    a = o @ sd["self_attn.out_proj.weight"].T + sd["self_attn.out_proj.bias"]
    y1, _, _ = KO.layernorm(a, x, sd["norm1.weight"], sd["norm1.bias"], 1e-5)
    f = KO.gelu(y1 @ sd["linear1.weight"].T + sd["linear1.bias"]) @ sd["linear2.weight"].T + sd["linear2.bias"]
    y2, _, _ = KO.layernorm(f, y1, sd["norm2.weight"], sd["norm2.bias"], 1e-5)
    assert _rel(y2, layer(x).detach()) <= 1e-12


# ----------------------------------------------------------------------------- modules, plugin, CLI
def test_cli_accepts_fbanks_kwt_with_vtlp_and_refuses_specaug():
    from speechrecognitionproject_amd.training import PLUGINS, SPECAUG_SHAPES, parse
    assert "fbanks_kwt" in PLUGINS and "fbanks_kwt" not in SPECAUG_SHAPES
    args = parse(["--model", "fbanks_kwt", "--vtlp", "0.9,1.1"])
    assert args.model == "fbanks_kwt" and args.vtlp == (0.9, 1.1)
    with pytest.raises(SystemExit):
        parse(["--model", "fbanks_kwt", "--specaug", "5,2,15,2,12"])


def test_restatement_and_plugin_state_dicts_agree():
    from speechrecognitionproject_amd.models import model_fbanks_kwt
    for kw in (dict(dim=64, heads=1, mlp_dim=128, layers=2), dict(dim=24, heads=3, mlp_dim=20, layers=1)):
        ref = {k: tuple(v.shape) for k, v in KO.FbanksKwt(**kw).state_dict().items()}
        sd = {k: tuple(v.shape) for k, v in model_fbanks_kwt.Network(**kw).state_dict().items()}
        assert sd == ref and list(sd) == list(ref)
    top = {k.split(".")[0] for k in sd}
    assert top == {"pos", "embed", "layers", "fc"} and sd["pos"] == (98, 24)
    assert len(model_fbanks_kwt.Network().layers) == 12     # KWT-1
    for name in ("DEVICE", "accuracy", "class_accuracy", "filter_banks", "Network"):
        assert hasattr(model_fbanks_kwt, name), name
    with pytest.raises(ValueError):
        model_fbanks_kwt.Network(vtlp=(0.5, 1.1))
    torch.manual_seed(1)
    pos = model_fbanks_kwt.Network(layers=1).pos.detach()
    assert abs(float(pos.std()) - 0.02) < 2e-3 and abs(float(pos.mean())) < 2e-3


@pytest.mark.parametrize("bad", [dict(dim=65, heads=2), dict(dim=256, heads=2), dict(dim=6, heads=1), dict(dim=8, heads=4)])
def test_constructor_refuses_head_sizes_outside_the_kernels_domain(bad):
    from speechrecognitionproject_amd import nn as snn
    from speechrecognitionproject_amd.models import model_fbanks_kwt
    with pytest.raises(ValueError):
        model_fbanks_kwt.Network(layers=1, **bad)
    with pytest.raises(ValueError):
        snn.MultiheadSelfAttention(bad["dim"], bad["heads"])


@pytest.mark.parametrize("dims", [(64, 1, 256), (24, 3, 20)])
def test_encoder_layer_state_dict_is_torchs_both_ways(dims):
    from speechrecognitionproject_amd import nn as snn
    torch.manual_seed(7)
    mine = snn.TransformerEncoderLayer(*dims)
    ref = torch.nn.TransformerEncoderLayer(*dims, dropout=0.0, activation="gelu", batch_first=True)
    assert [(k, tuple(v.shape)) for k, v in mine.state_dict().items()] == [(k, tuple(v.shape))
                                                                           for k, v in ref.state_dict().items()]
    ref.load_state_dict(mine.state_dict(), strict=True)
    for k, v in mine.state_dict().items():
        assert torch.equal(ref.state_dict()[k], v), k
    other = torch.nn.TransformerEncoderLayer(*dims, dropout=0.0, activation="gelu", batch_first=True)
    mine.load_state_dict(other.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(mine.state_dict()[k], v), k


def test_module_inits_are_torchs_under_the_same_seed():
    from speechrecognitionproject_amd import nn as snn
    pairs = [
        (lambda: snn.LayerNorm(20), lambda: torch.nn.LayerNorm(20)),
        (lambda: snn.MultiheadSelfAttention(24, 3), lambda: torch.nn.MultiheadAttention(24, 3, batch_first=True)),
        (lambda: snn.TransformerEncoderLayer(24, 3, 20),
         lambda: torch.nn.TransformerEncoderLayer(24, 3, 20, dropout=0.0, activation="gelu", batch_first=True)),
    ]
    for mine, ref in pairs:
        torch.manual_seed(11)
        a, after_a = mine(), torch.rand(3)
        torch.manual_seed(11)
        b, after_b = ref(), torch.rand(3)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(after_a, after_b)      # and the generator is where torch's constructor leaves it
    m = snn.LayerNorm(20, eps=1e-3)
    assert m.eps == 1e-3 and m.normalized_shape == (20,) and not list(snn.GELU().parameters())


# ----------------------------------------------------------------------------- host-side refusals
def _buf(n=4096):
    return (ctypes.c_float * n)()


GOOD = dict(B=2, H=2, T=7, dh=8)


def _mhsa_fwd(a, g):
    from speechrecognitionproject_amd import _lib
    _lib.call("srk_mhsa_fwd", a["qkv"], g["B"], g["H"], g["T"], g["dh"], 0.25, a["o"], a["lse"], None)


def _mhsa_bwd(a, g):
    from speechrecognitionproject_amd import _lib
    _lib.call("srk_mhsa_bwd", a["qkv"], a["lse"], a["do"], g["B"], g["H"], g["T"], g["dh"], 0.25, a["dqkv"], None)


def _mhsa_args():
    return {k: _buf() for k in ("qkv", "o", "lse", "do", "dqkv")}


MHSA_BAD = {"T0": dict(T=0), "T129": dict(T=129), "dh0": dict(dh=0), "dh6": dict(dh=6), "dh68": dict(dh=68),
            "H0": dict(H=0), "B0": dict(B=0), "T-1": dict(T=-1),
            "2^31": dict(B=1 << 13, H=1 << 4, T=128, dh=64),            # B T 3 H dh = 3 * 2^30
            "just-over": dict(B=(1 << 31) // (3 * 2 * 128 * 64) + 1, H=2, T=128, dh=64),
            "BH2^31": dict(B=1 << 20, H=1 << 11, T=1, dh=4),
            "overflow": dict(B=1 << 40, H=1 << 40, T=128, dh=64)}


@pytest.mark.parametrize("bad", list(MHSA_BAD))
def test_mhsa_rejects_values_outside_the_domain_on_the_host(bad):
    """Refused with "mhsa" in the message before any device work: host buffers stand in for the tensors, and there is
    no GPU here at all."""
    from speechrecognitionproject_amd import _lib
    g = dict(GOOD, **MHSA_BAD[bad])
    for run in (_mhsa_fwd, _mhsa_bwd):
        with pytest.raises(_lib.SrkError, match="mhsa"):
            run(_mhsa_args(), g)


def test_mhsa_rejects_null_pointers_and_a_scale_that_is_not_finite():
    from speechrecognitionproject_amd import _lib
    for run, names in ((_mhsa_fwd, ("qkv", "o", "lse")), (_mhsa_bwd, ("qkv", "lse", "do", "dqkv"))):
        for name in names:
            a = _mhsa_args()
            a[name] = None
            with pytest.raises(_lib.SrkError, match="mhsa"):
                run(a, GOOD)
    a = _mhsa_args()
    with pytest.raises(_lib.SrkError, match="mhsa"):
        _lib.call("srk_mhsa_fwd", a["qkv"], 2, 2, 7, 8, float("inf"), a["o"], a["lse"], None)


def _ln_args():
    return {k: _buf() for k in ("x", "res", "gamma", "beta", "y", "mean", "rstd", "dy", "ds", "dgamma", "dbeta", "ws")}


def _ln_fwd(a, M, D, eps=1e-5):
    from speechrecognitionproject_amd import _lib
    _lib.call("srk_layernorm_fwd", a["x"], a["res"], a["gamma"], a["beta"], M, D, eps, a["y"], a["mean"], a["rstd"],
              None)


def _ln_bwd(a, M, D):
    from speechrecognitionproject_amd import _lib
    _lib.call("srk_layernorm_bwd", a["x"], a["res"], a["gamma"], a["mean"], a["rstd"], a["dy"], M, D, a["ds"],
              a["dgamma"], a["dbeta"], 0.0, a["ws"], None)


@pytest.mark.parametrize("shape", [(5, 0), (5, 1025), (0, 64), (-1, 64), (1 << 21, 1024), (1 << 31, 1), (1 << 40, 1 << 40)],
                         ids=["D0", "D1025", "M0", "M-1", "2^31", "M2^31", "overflow"])
def test_layernorm_rejects_shapes_outside_the_domain_on_the_host(shape):
    from speechrecognitionproject_amd import _lib
    for run in (_ln_fwd, _ln_bwd):
        with pytest.raises(_lib.SrkError, match="layernorm"):
            run(_ln_args(), *shape)
    assert int(_lib.lib().srk_layernorm_workspace_floats(*shape)) == 0


def test_layernorm_rejects_each_required_null_pointer_on_the_host():
    from speechrecognitionproject_amd import _lib
    for run, names in ((_ln_fwd, ("x", "gamma", "beta", "y", "mean", "rstd")),
                       (_ln_bwd, ("x", "gamma", "mean", "rstd", "dy", "ds", "dgamma", "dbeta", "ws"))):
        for name in names:
            a = _ln_args()
            a[name] = None
            with pytest.raises(_lib.SrkError, match="layernorm"):
                run(a, 5, 64)
    for eps in (float("nan"), -1.0):
        with pytest.raises(_lib.SrkError, match="layernorm"):
            _ln_fwd(_ln_args(), 5, 64, eps)


def test_layernorm_workspace_is_positive_on_the_domain():
    from speechrecognitionproject_amd import _lib
    for shape in ((5, 64), (3, 130), (1, 1), (300, 192), (2, 1024), (7, 3), (512 * 98, 64), (1 << 20, 1024)):
        assert int(_lib.lib().srk_layernorm_workspace_floats(*shape)) > 0, shape


@pytest.mark.parametrize("n", [0, -3, 1 << 31, 1 << 40], ids=["n0", "n-3", "2^31", "2^40"])
def test_gelu_rejects_sizes_and_null_pointers_on_the_host(n):
    from speechrecognitionproject_amd import _lib
    with pytest.raises(_lib.SrkError, match="gelu"):
        _lib.call("srk_gelu_fwd", _buf(), n, _buf(), None)
    with pytest.raises(_lib.SrkError, match="gelu"):
        _lib.call("srk_gelu_bwd", _buf(), _buf(), n, _buf(), None)
    for nulls in ((None, 1), (1, None)):
        with pytest.raises(_lib.SrkError, match="gelu"):
            _lib.call("srk_gelu_fwd", nulls[0] and _buf(), 8, nulls[1] and _buf(), None)
    for nulls in ((None, 1, 1), (1, None, 1), (1, 1, None)):
        with pytest.raises(_lib.SrkError, match="gelu"):
            _lib.call("srk_gelu_bwd", nulls[0] and _buf(), nulls[1] and _buf(), 8, nulls[2] and _buf(), None)


def test_abi_declares_and_binds_the_new_symbols():
    from speechrecognitionproject_amd import _lib
    L = _lib.lib()
    for s in ("srk_mhsa_fwd", "srk_mhsa_bwd", "srk_layernorm_workspace_floats", "srk_layernorm_fwd",
              "srk_layernorm_bwd", "srk_gelu_fwd", "srk_gelu_bwd"):
        assert s in _lib.header_symbols() and s in _lib._SIGS and hasattr(L, s)
    assert L.srk_version() == _lib.ABI_VERSION == 3
