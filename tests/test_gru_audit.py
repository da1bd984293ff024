"""Host-side audit of the persistent GRU's step-ordering words (srk_gru_audit_words; no GPU): every
counter / flag word any workgroup of the planned launches polls, stores or adds to — computed with
the kernels' own index helpers (csrc/gru_internal.h pw_*) — lies below the XCD census, for every
kernel variant and for multi-chunk batches (b_begin > 0: the launch of rows 256..511 touches exactly
the words of the first launch).  VERDICT r02 #8: the round-2 scalar-poll experiment that faulted on
the two-chunk launch is not in the tree; this pins the shipped vector-poll path's addresses."""
import ctypes

import pytest

from speechrecognitionproject_amd import _lib


def _audit(B, prec, backward=0):
    mx, n, cen = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _lib.call("srk_gru_audit_words", B, prec, backward, ctypes.byref(mx), ctypes.byref(n), ctypes.byref(cen))
    return mx.value, n.value, cen.value


OPTS = [{"gru_fp32_dual_chain": 1, "gru_lp_32x32": 1, "gru_lp_wide": 1},
        {"gru_fp32_dual_chain": 1, "gru_lp_32x32": 1, "gru_lp_wide": 0},
        {"gru_fp32_dual_chain": 0, "gru_lp_32x32": 0, "gru_lp_wide": 0}]


@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_flag_words_below_census_and_chunk_independent(opts, prec):
    _check_flag_words(opts, prec, 0)


# The audit walks the launch plan itself (gru_rec_plan), so the backward pass's plans are pinned the same way.
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_flag_words_below_census_and_chunk_independent_backward(opts, prec):
    _check_flag_words(opts, prec, 1)


def _check_flag_words(opts, prec, backward):
    # 16-bit with gru_lp_wide: batches over 256 rows run as 512-row launches of 64-row workgroups
    wide = prec != 0 and opts["gru_lp_32x32"] and opts["gru_lp_wide"]
    with _lib.options(**opts):
        first = _audit(256, prec, backward)
        for B in (1, 63, 64, 200, 256, 300, 512, 1000, 4096):
            mx, n, cen = _audit(B, prec, backward)
            assert 0 <= mx < cen, (B, mx, cen)
            assert n == ((B + 511) // 512 if wide and B > 256 else (B + 255) // 256)
            if B % 256 == 0:
                assert mx == first[0]          # every full chunk touches the same words


# ------------------------------------------------------------------ workspace layout (csrc/gru.hip, struct GruWs)
def _up64(v):
    return (v + 63) // 64 * 64


def _layer_floats(B, T, IN, H, backward):
    """(floats up to the 16-bit block, floats of that block) of a layer workspace, written out from the layout's
    description: recurrence buffers | hand-off ring | 4096 step-ordering words | in4 pad block | 16-bit block."""
    BT, in4, in8 = B * T, (IN + 3) // 4 * 4, (IN + 7) // 8 * 8
    ring = 3 * min(_up64(B), 512) * H
    if backward:
        e = _up64(BT * 6 * H + 2 * BT * 3 * H + 2 * B * 3 * H + 2 * B * H) + 6 * ring
    else:
        e = _up64(BT * 6 * H + 2 * T * B * 4 * H) + 2 * ring
    e = _up64(e + 4096) + 64
    if IN % 4:
        e += BT * in4 + (2 if backward else 1) * 6 * H * in4 + 64
    if backward:
        blk = _up64((B + 255) // 256 * 8 * 2 * 4 * H) + (_up64(6 * H * in8) + _up64(BT * in8) if in8 != IN else 0)
    else:
        blk = _up64(BT * in8 // 2 + 1) + _up64(6 * H * in8 // 2 + 1) + _up64(BT * 2 * H // 2 + 1)
    return _up64(e), blk + 64


def test_workspace_layout_consistent():
    L = _lib.lib()
    Bs, Ts = (1, 63, 64, 65, 256, 257, 512, 513, 1000), (1, 2, 49)
    for IN in (1, 39, 40, 64, 65, 72, 1024):
        for H in (128, 512):
            for backward in (0, 1):
                size = {}
                for B in Bs:
                    for T in Ts:
                        n = int(L.srk_gru_workspace_floats(B, T, IN, H, backward))
                        top = int(L.srk_gru_top_last_workspace_floats(B, T, IN, H, backward))
                        # the top-last workspace: the layer's, plus in the backward the padded [B][T][2H] dy
                        assert top == n + (_up64(B * T * 2 * H) if backward else 0), (B, T, IN, H, backward)
                        # the 16-bit block is there exactly when H = 512
                        base, blk = _layer_floats(B, T, IN, H, backward)
                        assert n == base + (blk if H == 512 else 0), (B, T, IN, H, backward)
                        assert n % 64 == 0
                        size[B, T] = n
                # monotone in B and in T
                for i, B in enumerate(Bs):
                    for j, T in enumerate(Ts):
                        assert i == 0 or size[B, T] >= size[Bs[i - 1], T], (B, T, IN, H, backward)
                        assert j == 0 or size[B, T] >= size[B, Ts[j - 1]], (B, T, IN, H, backward)
