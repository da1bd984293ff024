"""Guard bands (tests/guarded.py) around every buffer of srk_mhsa_*, srk_layernorm_* and srk_gelu_*, by the three
runs of tests/test_guard_bands_gpu.py: ordinary tensors, then every pointer argument between two 64 KiB bands with the
caller-sized workspace exactly as large as its query says, pre-filled with zeros and with 0xFF bytes (NaN).  Asserted:
every band intact, no const input modified, every output finite, fully written and the plain run's bits whatever the
workspace held.  lead = 1 moves every tensor one element off its 16-byte alignment (the scalar paths)."""
import pytest
import torch

from guarded import WS_BYTES, Arena, band_value, same_bits
from speechrecognitionproject_amd import _lib

pytestmark = pytest.mark.gpu


def _never_written(t):
    iv, pat = band_value(t.dtype, "out")
    return int((t.contiguous().reshape(-1).view(iv) == pat).sum())


def run_case(fn):
    """fn(arena, outs) makes the case's calls and appends (name, tensor) to outs; returns the plain run's outputs."""
    runs = []
    for guarded, ws_byte in ((False, WS_BYTES[1]), (True, WS_BYTES[1]), (True, WS_BYTES[0])):
        a, o = Arena(guarded, ws_byte), []
        fn(a, o)
        a.check()
        runs.append([(n, t.detach().clone()) for n, t in o])
    plain = runs[0]
    for what, run in zip(("plain", "guarded, zeroed workspace", "guarded, 0xFF workspace"), runs):
        assert [n for n, _ in run] == [n for n, _ in plain]
        for (name, ref), (_, t) in zip(plain, run):
            assert bool(torch.isfinite(t).all()), "%s: non-finite (%s)" % (name, what)
            assert _never_written(t) == 0, "%s: %d elements never written (%s)" % (name, _never_written(t), what)
            assert same_bits(ref, t), "%s: differs from the plain run (%s)" % (name, what)
    return dict(plain)


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) + 1)


def _rn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


MHSA = [(2, 3, 7, 8), (2, 2, 1, 4), (2, 2, 65, 20), (2, 1, 128, 64), (3, 1, 98, 64)]   # B, H, T, dh


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("B,H,T,dh", MHSA)
def test_mhsa(gpu, B, H, T, dh, lead):
    D, scale = H * dh, dh ** -0.5

    def fn(a, o):
        g = _gen(B, H, T, dh)
        qkv = a.inp("qkv", _rn(g, B, T, 3 * D), lead=lead)
        out, lse = a.out("o", B * T * D, lead=lead), a.out("lse", B * H * T, lead=lead)
        a.call("srk_mhsa_fwd", qkv, B, H, T, dh, scale, out, lse)
        do = a.inp("do", _rn(g, B, T, D), lead=lead)
        dqkv = a.out("dqkv", B * T * 3 * D, lead=lead)
        a.call("srk_mhsa_bwd", qkv, lse, do, B, H, T, dh, scale, dqkv)
        o.extend([("o", out.t), ("lse", lse.t), ("dqkv", dqkv.t)])

    run_case(fn)


# M, D.  (4200, 64): the workspace's 1024 slabs; scalar slots (4 rows per workgroup) sweep twice, float4 slots (16
# rows) leave 761 workgroups without a row, which write zero slabs
LN = [(5, 64), (3, 130), (1, 1), (300, 192), (2, 1024), (7, 3), (4200, 64)]


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("acc_beta", [0.0, 1.0], ids=["write", "accumulate"])
@pytest.mark.parametrize("M,D", LN)
def test_layernorm(gpu, M, D, acc_beta, with_res, lead):
    nws = int(_lib.lib().srk_layernorm_workspace_floats(M, D))
    assert nws > 0 and nws % (2 * D) == 0

    def fn(a, o):
        g = _gen(M, D, with_res)
        x = a.inp("x", _rn(g, M, D) + 3.0, lead=lead)
        res = a.inp("res", _rn(g, M, D), lead=lead) if with_res else None
        gamma, beta = a.inp("gamma", 1.0 + _rn(g, D, scale=0.3), lead=lead), a.inp("beta", _rn(g, D), lead=lead)
        y, mean, rstd = a.out("y", M * D, lead=lead), a.out("mean", M, lead=lead), a.out("rstd", M, lead=lead)
        a.call("srk_layernorm_fwd", x, res, gamma, beta, M, D, 1e-5, y, mean, rstd)
        dy = a.inp("dy", _rn(g, M, D), lead=lead)
        ds = a.out("ds", M * D, lead=lead)
        init = (_rn(g, D), _rn(g, D)) if acc_beta else (None, None)
        dgamma, dbeta = a.out("dgamma", D, init=init[0], lead=lead), a.out("dbeta", D, init=init[1], lead=lead)
        a.call("srk_layernorm_bwd", x, res, gamma, mean, rstd, dy, M, D, ds, dgamma, dbeta, acc_beta,
               a.ws("ws", nws))
        o.extend([("y", y.t), ("mean", mean.t), ("rstd", rstd.t), ("ds", ds.t), ("dgamma", dgamma.t),
                  ("dbeta", dbeta.t)])

    run_case(fn)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1027, 4 * 256 * 3 + 2])
def test_gelu(gpu, n, lead):
    def fn(a, o):
        g = _gen(n)
        x = a.inp("x", _rn(g, n, scale=3.0), lead=lead)
        y = a.out("y", n, lead=lead)
        a.call("srk_gelu_fwd", x, n, y)
        dy = a.inp("dy", _rn(g, n), lead=lead)
        dx = a.out("dx", n, lead=lead)
        a.call("srk_gelu_bwd", x, dy, n, dx)
        o.extend([("y", y.t), ("dx", dx.t)])

    run_case(fn)
