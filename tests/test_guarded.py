"""The guard-band helper finds what it is there to find: stray writes made with plain torch indexing (no kernel is
involved), on whatever device is present."""
import pytest
import torch

from guarded import BAND, Arena, GuardError, Guarded, Plain, band_value, guarded_call, same_bits

DEV = "cuda" if torch.cuda.is_available() else "cpu"
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int16, torch.int32, torch.int64,
          torch.uint8]


@pytest.mark.parametrize("kind", ["in", "out", "ws"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", [0, 1, 3])
def test_untouched_bands_pass(kind, dtype, lead):
    g = Guarded(37, dtype, DEV, kind, lead=lead)
    assert g.t.numel() == 37 and g.t.dtype == dtype
    assert g.t.data_ptr() == g.data_ptr() == g.raw.data_ptr() + BAND + lead * g.es
    if lead == 0:
        assert g.data_ptr() % 16 == 0
    if kind == "in":
        g.set(torch.arange(37).to(dtype))
    else:
        g.t.copy_(torch.arange(37).to(dtype))      # an output may be written anywhere inside
    g.check("x")


@pytest.mark.parametrize("kind", ["in", "out", "ws"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int64, torch.uint8])
def test_one_element_past_the_end_raises(kind, dtype):
    g = Guarded(10, dtype, DEV, kind, lead=1)
    off = g.front + g.nbytes
    g.raw[off:off + g.es].view(dtype)[0] = 1       # the element after the interior
    with pytest.raises(GuardError, match=r"`y`: \d+ B written past the end"):
        g.check("y")


@pytest.mark.parametrize("kind", ["in", "out", "ws"])
@pytest.mark.parametrize("lead", [0, 1])
def test_one_byte_before_the_start_raises(kind, lead):
    g = Guarded(10, torch.float32, DEV, kind, lead=lead)
    g.raw[g.front - 1] = 0
    with pytest.raises(GuardError, match="`y`: 1 B written before the start"):
        g.check("y")


def test_distance_is_reported():
    g = Guarded(8, torch.float32, DEV, "out")
    g.raw[g.front + g.nbytes + 12:g.front + g.nbytes + 16] = 0     # bytes 13..16 past the end
    with pytest.raises(GuardError, match="`y`: 13 B written past the end"):
        g.check("y")
    h = Guarded(8, torch.float32, DEV, "out")
    h.raw[0] = 0                                                    # the far edge of the front band
    with pytest.raises(GuardError, match="`y`: %d B written before the start" % BAND):
        h.check("y")


def test_write_into_an_input_raises():
    g = Guarded(10, torch.float32, DEV, "in").set(torch.ones(10))
    g.check("x")
    g.t[3] = 2.0
    with pytest.raises(GuardError, match="`x`: const input modified"):
        g.check("x")


def test_band_contents():
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        g = Guarded(4, dtype, DEV, "in")
        band = g.raw[:BAND].view(dtype)
        assert bool(torch.isnan(band).all())                       # a stray read enters arithmetic as NaN
        o = Guarded(4, dtype, DEV, "out")
        assert bool(torch.isfinite(o.raw.view(dtype)).all()) and bool((o.raw != 0).all())
        assert bool((o.t.view(torch.uint8) == 0x5A).all())         # a never-written element shows
    assert band_value(torch.int16, "in")[1] == 32767
    assert band_value(torch.int32, "in")[1] == -1 and band_value(torch.int64, "in")[1] == -1
    assert band_value(torch.uint8, "in")[1] == 0xFF
    assert bool((Guarded(6, torch.float32, DEV, "ws", ws_byte=0xFF).t.view(torch.uint8) == 0xFF).all())
    assert bool((Guarded(6, torch.float32, DEV, "ws", ws_byte=0).t.view(torch.uint8) == 0).all())


def test_arena_checks_every_buffer_and_plain_is_the_same_interface():
    for guarded in (True, False):
        a = Arena(guarded, device=DEV)
        x = a.inp("x", torch.arange(6.0).view(2, 3), lead=1)
        y = a.out("y", 6)
        w = a.ws("ws", 5)
        assert isinstance(x, Guarded if guarded else Plain)
        assert torch.equal(x.t.cpu(), torch.arange(6.0)) and y.t.numel() == 6 and w.t.numel() == 5
        y.t.copy_(x.t)
        a.check()
    a = Arena(True, device=DEV)
    a.inp("x", torch.zeros(4))
    w = a.ws("ws", 5)
    w.raw[w.front + w.nbytes] = 1
    with pytest.raises(GuardError, match="`ws`: 1 B written past the end"):
        a.check()


def test_same_bits():
    nan1 = torch.tensor([0x7FC00001], dtype=torch.int32).view(torch.float32)
    nan2 = torch.tensor([0x7FC00002], dtype=torch.int32).view(torch.float32)
    assert same_bits(nan1, nan1.clone()) and not same_bits(nan1, nan2)
    assert not same_bits(torch.zeros(2), -torch.zeros(2))
    assert same_bits(torch.empty(0), torch.empty(0))


@pytest.mark.gpu
def test_guarded_call_runs_an_entry_point(gpu):
    x = torch.randn(5, 7)
    for guarded in (True, False):
        (y,) = guarded_call("srk_colsum_f32", [("in", x.cuda()), 5, 7, 7, ("out", 7, torch.float32), 0.0], guarded)
        assert (y.cpu().double() - x.double().sum(0)).abs().max() <= 5 * 2.0 ** -23 * x.abs().sum(0).max()
