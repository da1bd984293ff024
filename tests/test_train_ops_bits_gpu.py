"""The training-step ops (Adam, cross-entropy, dropout mask) against tests/golden/train_ops_bits.json, bit for bit.

The record was made by tools/train_ops_bits.py from the commit before the Adam updates, the cross-entropy row kernels
and the mask kernels became one each; it is the anchor from outside the code under test (the features-off tests of
test_optim_ext_gpu.py and test_mixup_gpu.py compare a kernel with itself).  Every case of the record is recomputed
once with the working tree's library, and every digest has to be equal.  The Adam and dropout digests hold under any
toolchain; the cross-entropy ones go through expf / logf and are bound to the ROCm install of the record (its "note"
says how to re-record)."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "train_ops_bits.json")) as _f:
    GOLDEN = json.load(_f)


@functools.lru_cache(maxsize=None)
def _computed():
    spec = importlib.util.spec_from_file_location("train_ops_bits",
                                                  os.path.join(os.path.dirname(HERE), "tools", "train_ops_bits.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.compute()


def test_the_record_is_complete(gpu):
    """Every case the tool computes is in the record and the other way round: none can drop out unnoticed."""
    assert sorted(_computed()) == sorted(GOLDEN["cases"])
    assert len(GOLDEN["cases"]) == 6 * 5 + 2 * 4 + 2 * 2


@pytest.mark.parametrize("case", sorted(GOLDEN["cases"]))
def test_bits(gpu, case):
    want, got = GOLDEN["cases"][case], _computed()[case]
    assert got["inputs_sha256"] == want["inputs_sha256"], \
        "%s: the inputs differ from the record's (the host random number generator, not the kernels)" % case
    assert sorted(got["outputs"]) == sorted(want["outputs"])
    for name, w in want["outputs"].items():
        g = got["outputs"][name]
        for part in ("bits", "head", "tail"):      # the words the record keeps, to look at a mismatch
            if g["sha256"] != w["sha256"] and part in w:
                diff = [(i, a, b) for i, (a, b) in enumerate(zip(g[part], w[part])) if a != b]
                print("%s %s: %d of the %d words of %r differ; first (index, got, recorded): %s"
                      % (case, name, len(diff), len(w[part]), part, [(i, hex(a), hex(b)) for i, a, b in diff[:8]]))
        assert g["sha256"] == w["sha256"], "%s: %s differs from the recorded bits" % (case, name)
