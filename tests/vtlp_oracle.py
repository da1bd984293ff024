"""Float64 numpy restatement of the reference's VTLP-warped filter bank — TEST INFRASTRUCTURE ONLY.

legacy/model_8/dataset_top.py:245-267: the fbank front end of models/model_fbanks_cnn.py (restated in
oracle.features.filter_banks) with the 122 mel points warped by a per-clip factor alpha before they are
turned into FFT bins.  Everything up to the power spectrum is oracle.features' arithmetic; only the mel
matrix differs.  Also the draw of the warp factors (srk_uniform_f64_state) in Python integers / floats.
"""
import numpy as np

from oracle import features as OF


def hz_points():
    nfilt, sr = OF.FB_NFILT, OF.SR
    high_freq_mel = 2595 * np.log10(1 + (sr / 2) / 700)            # dataset_top.py:247
    mel_points = np.linspace(0, high_freq_mel, nfilt + 2)           # :248
    return 700 * (10 ** (mel_points / 2595) - 1)                    # :249


def warped_bins(alpha):
    """float64[122]: floor((NFFT + 1) * warped hz / sr), dataset_top.py:252-254 in its operation order."""
    alpha = float(alpha)
    hz = hz_points()
    m = min(alpha, 1)
    knee = 4800 * m / alpha
    s = (8000 - 4800 * m) / (8000 - 4800 * (m / alpha))
    hzw = np.array([hz[i] * alpha if hz[i] < knee else 8000 - s * (8000 - hz[i]) for i in range(len(hz))])
    return np.floor((OF.FB_NFFT + 1) * hzw / OF.SR)


def warped_fbank_matrix(alpha):
    """float64[120, 257], dataset_top.py:256-264."""
    nfilt = OF.FB_NFILT
    bins = warped_bins(alpha)
    fbank = np.zeros((nfilt, OF.FB_NFFT // 2 + 1))
    for m in range(1, nfilt + 1):
        f_m_minus, f_m, f_m_plus = int(bins[m - 1]), int(bins[m]), int(bins[m + 1])
        for k in range(f_m_minus, f_m):
            fbank[m - 1, k] = (k - bins[m - 1]) / (bins[m] - bins[m - 1])
        for k in range(f_m, f_m_plus):
            fbank[m - 1, k] = (bins[m + 1] - k) / (bins[m + 1] - bins[m])
    return fbank


def filter_banks_vtlp(sample, alpha):
    """float32[16000] PCM -> float32[98, 120] dB with the mel matrix warped by alpha: the statements of
    oracle.features.filter_banks with warped_fbank_matrix(alpha) in place of the constant matrix."""
    signal = np.asarray(sample, dtype=np.float32)
    emph = np.append(signal[0], signal[1:] - np.float32(OF.FB_PRE_EMPHASIS) * signal[:-1])
    pad_len = OF.FB_NUM_FRAMES * OF.FB_FRAME_STEP + OF.FB_FRAME_LEN
    pad = np.append(emph, np.zeros(pad_len - len(emph)))
    frames = pad[OF.fbank_frame_index()] * np.hamming(OF.FB_FRAME_LEN)
    mag = np.abs(np.fft.rfft(frames, OF.FB_NFFT))
    pow_frames = (1.0 / OF.FB_NFFT) * mag ** 2
    fb = pow_frames @ warped_fbank_matrix(alpha).T                                       # :265
    fb = np.where(fb == 0, np.finfo(float).eps, fb)                                      # :266
    return (20 * np.log10(fb)).astype(np.float32)                                        # :267


EPS_DB = np.float32(20 * np.log10(np.finfo(float).eps))

_M64 = (1 << 64) - 1


def uniform_f64(base, counter, n, lo, hi):
    """srk_uniform_f64_state's draws for the state {base, counter}: float64[n]."""
    seed = (base + 0xD1B54A32D192ED03 * counter) & _M64
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        z ^= z >> 31
        u = float(z >> 11) * 2.0 ** -53
        out[i] = float(lo) + (float(hi) - float(lo)) * u
    return out
