"""The zero-block packing plan (srk_gemm_pack_plan), read without a GPU.

The last-step top BiGRU layer's reverse-direction dW_ih GEMM has B live k rows, (b, T-1), among B T; the plan keeps
the 8-aligned k blocks that hold one, slab by slab of the full GEMM's K split, and pads every slab with zero blocks
to a common length that is a multiple of 16.  The numpy side restates that from the definition: it lists
{(b T + T-1) // 8}, groups the blocks by 8 kb // slab and pads.  The entry point reads its answer back through the
function the gather kernel runs (PackPlan::src), so agreement here is agreement of what the kernel gathers."""
import ctypes

import numpy as np
import pytest

from speechrecognitionproject_amd import _lib


def restate(B, T, slab):
    K = B * T
    nslabs = -(-K // slab)
    blocks = np.unique((np.arange(B) * T + T - 1) // 8)
    owner = 8 * blocks // slab
    slabs = [[int(kb) for kb in blocks[owner == s]] for s in range(nslabs)]
    pslab = -(-max(8 * len(s) for s in slabs) // 16) * 16
    return slabs, pslab


# (B, T, slab).  T in {16, 17, 51}; B T no multiple of 8 (3 x 17, 5 x 51, 24 x 17 / 96, ...); a slab without a live
# row (B = 2: the rows T-1 and 2 T - 1 leave whole slabs of 16 empty); the live row B T - 1 in the last, partial 8-block
# (3 x 17 = 51, 2 x 51 = 102, 65 x 19); the benchmark's top layer (256, 51) at its slab of 2624; one slab for all of K.
CASES = [(20, 16, 64), (24, 17, 96), (65, 19, 256), (256, 51, 2624), (3, 17, 16), (5, 51, 32), (2, 16, 16), (2, 17, 16),
         (2, 51, 16), (1, 16, 16), (7, 51, 368), (24, 17, 416), (33, 16, 48)]


@pytest.mark.parametrize("B,T,slab", CASES)
def test_plan_matches_numpy_restatement(B, T, slab):
    want, want_pslab = restate(B, T, slab)
    got, pslab = _lib.gemm_pack_plan(B * T, slab, T - 1, T, B)
    assert got == want
    assert pslab == want_pslab and pslab % 16 == 0 and pslab >= 16
    assert sum(len(s) for s in got) == B            # T >= 8: every live row has an 8-block of its own
    for s, blocks in enumerate(got):                # a kept block stays inside the slab its k came from
        assert all(s * slab <= 8 * kb < (s + 1) * slab for kb in blocks)
        assert 8 * len(blocks) <= pslab


def test_cases_cover_what_they_claim():
    assert {T for _, T, _ in CASES} >= {16, 17, 51}
    assert any((B * T) % 8 for B, T, _ in CASES)
    assert any(B == 2 and any(not s for s in restate(B, T, slab)[0]) for B, T, slab in CASES)
    # the last live row, B T - 1, in a block that runs past K
    assert any((B * T) % 8 and restate(B, T, slab)[0][-1][-1] * 8 + 8 > B * T for B, T, slab in CASES)


@pytest.mark.parametrize("K,slab,first,stride,count", [
    (0, 16, 0, 16, 1),        # no K
    (64, 0, 15, 16, 4),       # no slab
    (64, 24, 15, 16, 4),      # a slab that is no multiple of 16
    (64, 8, 15, 16, 4),
    (64, -16, 15, 16, 4),
    (64, 16, -1, 16, 4),      # a negative first row
    (64, 16, 7, 7, 4),        # two live rows could share an 8-block
    (64, 16, 15, 16, 0),      # no live row
    (64, 16, 15, 16, 5),      # the last live row at 79 >= K
    (64, 16, 64, 16, 1),
])
def test_bad_arguments_are_refused(K, slab, first, stride, count):
    with pytest.raises(_lib.SrkError, match="pack_plan"):
        _lib.gemm_pack_plan(K, slab, first, stride, count)


def test_short_buffers_and_null_pointers_are_refused():
    L = _lib.lib()
    blocks, counts = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    n, ps = ctypes.c_int64(0), ctypes.c_int64(0)
    ok = (64, 16, 15, 16, 4)
    assert L.srk_gemm_pack_plan(*ok, blocks, 4, counts, 4, ctypes.byref(n), ctypes.byref(ps)) == 0
    assert (n.value, ps.value, list(blocks), list(counts)) == (4, 16, [1, 3, 5, 7], [1, 1, 1, 1])
    assert L.srk_gemm_pack_plan(*ok, blocks, 3, counts, 4, ctypes.byref(n), ctypes.byref(ps)) != 0
    assert b"room" in L.srk_last_error()
    assert L.srk_gemm_pack_plan(*ok, blocks, 4, counts, 3, ctypes.byref(n), ctypes.byref(ps)) != 0
    assert b"room" in L.srk_last_error()
    assert L.srk_gemm_pack_plan(*ok, None, 4, counts, 4, ctypes.byref(n), ctypes.byref(ps)) != 0
    assert b"null" in L.srk_last_error()
    assert L.srk_gemm_pack_plan(*ok, blocks, 4, counts, 4, None, ctypes.byref(ps)) != 0
    assert b"null" in L.srk_last_error()
