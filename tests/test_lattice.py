"""tests/lattice.py on the CPU: conditions on the REFERENCE alone that every conv + pool case of
tests/test_special_values_gpu.py has to meet, so that a bitwise comparison against it is possible (fp32 and float64
agree exactly, the operands are exact in bf16 and fp16) and cannot pass vacuously (enough windows hold exact ties,
with and without position 0 among the maxima)."""
import pytest
import torch

import lattice as L

IDS = ["x".join(str(v) for v in k) for k in L.all_keys()]


@pytest.mark.parametrize("key", L.all_keys(), ids=IDS)
def test_reference_is_exact(key):
    case = L.conv_pool_case(*key)
    for a, c in zip(case["ref32"], case["ref64"]):
        assert a.dtype in (torch.float32, torch.uint8)
        assert torch.equal(a.double(), c.double())           # same bits after the exact widening
    for name in ("x", "w", "b", "gy"):
        assert L.exact16(case[name]), name
    assert int(case["arg"].max()) < key[-1]


@pytest.mark.parametrize("key", L.all_keys(), ids=IDS)
def test_ties_are_there(key):
    N, H, W, Ci, Co, KH, KW, ph, pw, pool = key
    cen = L.conv_pool_case(*key)["census"]
    tied, inter = cen["tied"], cen["interior"]
    per_clip = tied.flatten(1).float().mean(1)
    no0 = int(cen["tied_no0"].sum())
    print("%s: %.1f %% of %d windows tied, per clip %s, %d tied away from position 0"
          % (key, 100 * tied.float().mean(), tied.numel(), ["%.1f %%" % (100 * v) for v in per_clip], no0))
    assert tied.float().mean() >= 0.25
    # one clip with every interior window tied (all windows, where no window is clear of the border), one with few
    assert any(bool(tied[n][inter[n]].all()) and (bool(inter[n].any()) or bool(tied[n].all())) for n in range(N))
    assert float(per_clip.min()) < 0.05
    Wo = W + 2 * pw - KW + 1
    if Wo >= 3 * KW:   # (narrower maps, the tiny split-K shape among them, have no room for such windows)
        assert no0 >= 16


def test_pool_cases_tie():
    for shape in ((2, 98, 12, 8), (2, 5, 8, 4)):
        for kh, kw in ((1, 3), (1, 4), (98, 1), (2, 1)):
            if shape[1] < kh:
                continue
            case = L.pool_case(*shape, kh, kw)
            x = case["x"]
            N, H, W, C = x.shape
            win = x[:, :H // kh * kh, :W // kw * kw].reshape(N, H // kh, kh, W // kw, kw, C)
            mx = win.amax(dim=(2, 4), keepdim=True)
            tied = (win == mx).sum(dim=(2, 4)) >= 2
            assert tied.float().mean() >= 0.25 and L.exact16(x) and L.exact16(case["gy"])
            # the gradient of a tied window lands on ONE element: the reference's dx holds gy's values once each
            assert torch.equal(case["dx"].abs().sum(), case["gy"].abs().sum())
