"""VTLP-warped filter bank (legacy/model_8/dataset_top.py:245-267) on the CPU: the float64 restatement
against the pinned unwarped one, and srk_vtlp_bins — the host entry that evaluates the kernel's own
`__host__ __device__` bin function — against the restatement, bin for bin.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from oracle import features as OF
from vtlp_oracle import filter_banks_vtlp, uniform_f64, warped_bins, warped_fbank_matrix
from speechrecognitionproject_amd import _lib


def lib_bins(alpha):
    b = (ctypes.c_int32 * 122)()
    rc = _lib.lib().srk_vtlp_bins(float(alpha), b)
    return rc, np.array(b[:], dtype=np.int64)


def test_unwarped_matrix_is_the_fbank_matrix():
    assert np.array_equal(warped_fbank_matrix(1.0), OF.fbank_matrix())


def test_unwarped_features_are_the_pinned_filter_banks():
    g = golden("fbank_golden.npz")
    for c in g["pcm"]:
        a, b = filter_banks_vtlp(c, 1.0), OF.filter_banks(c)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_warped_bins_shape_over_the_domain():
    # monotone, inside the spectrum, ends fixed: what the kernel's run-time tap bounds rely on
    for a in np.linspace(0.8, 1.25, 451):
        b = warped_bins(a)
        assert (np.diff(b) >= 0).all() and b[0] == 0 and b[-1] == 256, a
        assert (b[2:] - b[:-2]).max() <= 15, a


def _alphas():
    rng = np.random.default_rng(20260)
    return np.concatenate([
        [0.8, 0.9, 1.0, 1.1, 1.25, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)],
        np.linspace(0.8, 1.25, 2001),
        rng.uniform(0.9, 1.1, 2000),
    ])


def test_library_bins_equal_the_restatement():
    bad = []
    for a in _alphas():
        rc, b = lib_bins(a)
        assert rc == 0, (a, _lib.lib().srk_last_error())
        if not np.array_equal(b, warped_bins(a).astype(np.int64)):
            bad.append(float(a))
    assert not bad, bad[:10]


@pytest.mark.parametrize("alpha", [0.79, 1.26, float("nan"), float("inf"), 0.0])
def test_library_bins_reject_alpha_outside_the_domain(alpha):
    rc, _ = lib_bins(alpha)
    assert rc == -1 and b"alpha" in _lib.lib().srk_last_error()


def test_library_bins_reject_null():
    assert _lib.lib().srk_vtlp_bins(1.0, None) == -1


def test_new_entry_points_validate_before_device_work():
    L = _lib.lib()
    assert L.srk_fbank_vtlp_fwd(None, -1, None, None, None) == -1
    assert L.srk_fbank_vtlp_fwd_i16(None, -1, None, None, None) == -1
    assert L.srk_uniform_f64_state(None, 0.9, 1.1, 4, None, None) == -1
    assert L.srk_uniform_f64_state(ctypes.c_void_p(64), 1.1, 0.9, 4, ctypes.c_void_p(64), None) == -1


def test_uniform_oracle_known_properties():
    u = uniform_f64(1234, 0, 4096, 0.9, 1.1)
    assert u.min() >= 0.9 and u.max() < 1.1 and abs(u.mean() - 1.0) < 0.01
    assert not np.array_equal(u[:5], uniform_f64(1234, 1, 5, 0.9, 1.1))


def test_training_cli_vtlp_flag():
    from speechrecognitionproject_amd.training import parse
    assert parse(["--model", "fbanks_cnn"]).vtlp is None
    assert parse(["--model", "fbanks_cnn", "--vtlp", "0.9,1.1"]).vtlp == (0.9, 1.1)
    for argv in (["--model", "mfcc_bgru", "--vtlp", "0.9,1.1"], ["--vtlp", "0.9,1.1"],
                 ["--model", "fbanks_cnn", "--vtlp", "0.9"], ["--model", "fbanks_cnn", "--vtlp", "0.5,1.1"]):
        with pytest.raises(SystemExit):
            parse(argv)
