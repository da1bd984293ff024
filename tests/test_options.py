"""The runtime options (csrc/options.h: srk_set_option / srk_get_option / srk_option_list, _lib.options), no GPU.

options_table.json is the record of the library BEFORE the options became one table: tools/options_probe.py offered
every public name the values in "probes" through srk_set_option and wrote down which were accepted; the defaults are
transcribed from that library's definitions.  The table must have exactly those names and defaults and accept
exactly those values.  "release_scratch" (an action that synchronizes the device) is never called here."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from speechrecognitionproject_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = json.load(open(os.path.join(HERE, "options_table.json")))
OPTIONS = RECORD["options"]
VALUED = [n for n, o in OPTIONS.items() if o["default"] is not None]


@pytest.fixture(autouse=True)
def _state_put_back():
    """Every test leaves the options (and the Python mirror of matmul_precision) as it found them."""
    before = {n: o["current"] for n, o in _lib.option_table().items() if o["current"] is not None}
    yield
    for n, v in before.items():
        _lib.set_option(n, v)


def _get(name):
    v = ctypes.c_int64(-12345)
    assert _lib.lib().srk_get_option(name.encode(), ctypes.byref(v)) == 0
    return int(v.value)


def _normal_form(name, v):
    """What srk_get_option returns after srk_set_option(name, v) was accepted."""
    o = OPTIONS[name]
    if len(o["probes"]) > 1 and o["accepted"] == o["probes"]:   # a boolean: every value accepted, stored as v != 0
        return int(v != 0)
    if name == "gru_dwhh_fused":
        return v if v & 1 else 0
    if name == "gru_dc_offset_ns":
        return v // 10 * 10
    return v


def _child(code, **env):
    e = {k: v for k, v in os.environ.items() if k != "SRK_OPTIONS"}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_table_has_the_recorded_names_and_defaults():
    need = ctypes.c_int64(0)
    _lib.call("srk_option_list", None, 0, ctypes.byref(need))
    buf = ctypes.create_string_buffer(int(need.value))
    _lib.call("srk_option_list", buf, len(buf), ctypes.byref(need))
    lines = buf.value.decode().splitlines()
    names = [line.split("\t")[0] for line in lines]
    assert all(len(line.split("\t")) == 5 and line.split("\t")[4] for line in lines)   # name, default, current, accepts, doc
    assert len(names) == len(set(names)) and sorted(names) == sorted(OPTIONS)
    table = _lib.option_table()
    assert list(table) == names
    for n, o in OPTIONS.items():
        assert table[n]["default"] == o["default"], n
    assert table["release_scratch"]["accepts"] == "action" and table["release_scratch"]["current"] is None


def test_fresh_process_runs_at_the_defaults():
    got = _child("import json; from speechrecognitionproject_amd import _lib; "
                 "print(json.dumps({n: [o['default'], o['current']] for n, o in _lib.option_table().items()}))")
    assert sorted(got) == sorted(OPTIONS)
    for n, (default, current) in got.items():
        assert default == current == OPTIONS[n]["default"], n


@pytest.mark.parametrize("name", VALUED)
def test_accepts_and_stores_what_the_record_says(name):
    L = _lib.lib()
    o = OPTIONS[name]
    assert o["probes"]
    for v in o["probes"]:
        before = _get(name)
        rc = L.srk_set_option(name.encode(), v)
        assert (rc == 0) == (v in o["accepted"]), (name, v, rc)
        if rc == 0:
            assert _get(name) == _normal_form(name, v), (name, v)
            # the value read back sets the same state again
            assert L.srk_set_option(name.encode(), _get(name)) == 0 and _get(name) == _normal_form(name, v), (name, v)
        else:
            assert rc == -1 and _get(name) == before, (name, v)
            msg = L.srk_last_error().decode()
            assert name in msg and str(v) in msg, msg


def test_options_restores_on_exit_and_on_exception():
    _lib.set_option("conv_ring", 0x37)
    with _lib.options(conv_ring=0x87, conv_tile=256):
        assert (_lib.option("conv_ring"), _lib.option("conv_tile")) == (0x87, 256)
    assert (_lib.option("conv_ring"), _lib.option("conv_tile")) == (0x37, 128)
    with pytest.raises(ZeroDivisionError):
        with _lib.options(conv_ring=6, gru_dc_offset_ns=55):
            assert (_lib.option("conv_ring"), _lib.option("gru_dc_offset_ns")) == (6, 50)
            1 / 0
    assert (_lib.option("conv_ring"), _lib.option("gru_dc_offset_ns")) == (0x37, 2000)


def test_options_puts_back_what_it_set_when_a_later_value_is_refused():
    ran = []
    with pytest.raises(_lib.SrkError):
        with _lib.options(conv_ring_qs=1, gemm16_kernel=2, conv_tile=129, bn_tree=1):
            ran.append(1)
    assert not ran
    assert [_lib.option(n) for n in ("conv_ring_qs", "gemm16_kernel", "conv_tile", "bn_tree")] == [6, 0, 128, 0]


def test_options_nests():
    with _lib.options(conv_ring=6, mfcc_variant=1):
        with _lib.options(conv_ring=0x87):
            with _lib.options(conv_ring=0, mfcc_variant=2):
                assert (_lib.option("conv_ring"), _lib.option("mfcc_variant")) == (0, 2)
            assert (_lib.option("conv_ring"), _lib.option("mfcc_variant")) == (0x87, 1)
        assert (_lib.option("conv_ring"), _lib.option("mfcc_variant")) == (6, 1)
    assert (_lib.option("conv_ring"), _lib.option("mfcc_variant")) == (0x77, 3)


def test_scope_returns_to_the_srk_options_setting_not_the_default():
    got = _child("import json; from speechrecognitionproject_amd import _lib\n"
                 "seen = [_lib.option('conv_ring')]\n"
                 "with _lib.options(conv_ring=0x77):\n"
                 "    with _lib.options(conv_ring=0x87):\n"
                 "        seen.append(_lib.option('conv_ring'))\n"
                 "    seen.append(_lib.option('conv_ring'))\n"
                 "seen.append(_lib.option('conv_ring'))\n"
                 "print(json.dumps(seen))", SRK_OPTIONS="conv_ring=6")
    assert got == [6, 0x87, 0x77, 6]


def test_matmul_precision_mirror_follows_set_option():
    assert _lib.matmul_precision() == "fp32" and _lib.option("matmul_precision") == 0
    _lib.set_option("matmul_precision", 1)
    assert _lib.matmul_precision() == "bf16" and _lib.option("matmul_precision") == 1
    with pytest.raises(_lib.SrkError):
        _lib.set_option("matmul_precision", 3)
    assert _lib.matmul_precision() == "bf16" and _lib.option("matmul_precision") == 1
    with _lib.options(matmul_precision=2):
        assert _lib.matmul_precision() == "fp16"
    assert _lib.matmul_precision() == "bf16"
    with _lib.precision_scope("fp32"):
        assert _lib.matmul_precision() == "fp32" and _lib.option("matmul_precision") == 0
    assert _lib.matmul_precision() == "bf16" and _lib.option("matmul_precision") == 1
    _lib.set_matmul_precision("fp32")
    assert _lib.matmul_precision() == "fp32" and _lib.option("matmul_precision") == 0


def test_unknown_names_and_the_action_are_refused():
    with pytest.raises(_lib.SrkError, match="unknown option"):
        _lib.set_option("no_such_option", 0)
    assert RECORD["unknown_name"] == {"status": -1, "error": _lib.lib().srk_last_error().decode()}
    with pytest.raises(_lib.SrkError, match="unknown option"):
        _lib.option("gru_lp2")   # the variable's name, not the public one
    L = _lib.lib()
    v = ctypes.c_int64(7)
    assert L.srk_get_option(b"release_scratch", ctypes.byref(v)) == -1 and v.value == 7
    assert L.srk_get_option(b"conv_ring", None) == -1
    assert L.srk_get_option(None, ctypes.byref(v)) == -1 and v.value == 7
    with pytest.raises(_lib.SrkError):
        with _lib.options(release_scratch=1):
            pass
