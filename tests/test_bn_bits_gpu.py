"""The BatchNorm entry points (csrc/bn.hip) against tests/golden/bn_bits.json, bit for bit.

The record was made by tools/bn_bits.py from the commit before bn.hip got one reduction plan, one launcher per
reduction and one element launcher; it is the anchor from outside the code under test (test_bn_finalize_gpu.py and
test_bn_copy16_gpu.py compare the library with itself or with a tolerance).  Every case of the record is recomputed
once with the working tree's library, and every digest has to be equal.  The digests go through 1 / sqrtf and
expressions the compiler contracts, so they are bound to the ROCm install of the record (its "note" says how to
re-record)."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "bn_bits.json")) as _f:
    GOLDEN = json.load(_f)


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("bn_bits", os.path.join(os.path.dirname(HERE), "tools", "bn_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@functools.lru_cache(maxsize=None)
def _computed():
    return _tool().compute()


def test_the_record_is_complete(gpu):
    """Every case the tool computes is in the record and the other way round: none can drop out unnoticed."""
    assert sorted(_computed()) == sorted(GOLDEN["cases"])
    assert len(GOLDEN["cases"]) == _tool().case_count() == 12 * 18 + 4 * 12


@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_bits(gpu, case):
    want, got = GOLDEN["cases"][case], _computed()[case]
    assert got["inputs_sha256"] == want["inputs_sha256"], \
        "%s: the inputs differ from the record's (the host random number generator, not the kernels)" % case
    assert sorted(got["outputs"]) == sorted(want["outputs"])
    for name, w in want["outputs"].items():
        g = got["outputs"][name]
        if g["sha256"] != w["sha256"] and "bits" in w:      # the words the record keeps, to look at a mismatch
            diff = [(i, a, b) for i, (a, b) in enumerate(zip(g["bits"], w["bits"])) if a != b]
            print("%s %s: %d of the %d words differ; first (index, got, recorded): %s"
                  % (case, name, len(diff), len(w["bits"]), [(i, hex(a), hex(b)) for i, a, b in diff[:8]]))
        assert g["sha256"] == w["sha256"], "%s: %s differs from the recorded bits" % (case, name)
