"""Float64 restatement of the MFCC feature, the definition csrc/mfcc.hip is held to.

TEST INFRASTRUCTURE ONLY.  The reference calls librosa.feature.mfcc(audio, sr, n_mfcc, n_fft, hop_length) with librosa 0.8.0's
defaults (neural_waveshaping_synthesis/data/utils/mfcc_extraction.py:7-13); librosa is not installed, so its documented chain is
restated here and parity with librosa itself is UNPINNED:
  melspectrogram: |stft(y, n_fft, hop, hann, center / reflect)|^2, filters.mel(sr, n_fft, n_mels 128, fmin 0, fmax sr / 2,
      htk False, norm "slaney")
  power_to_db(S, ref 1, amin 1e-10, top_db 80): 10 log10(max(amin, S)), then max(., max(.) - top_db) over the whole array
  scipy.fftpack.dct(., axis 0, type 2, norm "ortho")[:n_mfcc]
The STFT is oracle/loudness_oracle.stft_magnitude (pinned against torch.stft and scipy.signal.stft in
tests/test_oracle_loudness.py).  tests/test_cpu_mfcc.py checks the filter bank against transformers.audio_utils.mel_filter_bank and
the DCT matrix against scipy.fftpack.dct.

`mfcc_float32` is the same chain in float32 arithmetic with the windowed DFT as a matrix product (sums of n_fft fp32 terms,
the kernel's kind of transform): its distance from the float64 result is the yardstick of tests/test_gpu_mfcc.py.
"""
import numpy as np

from oracle.loudness_oracle import hann_periodic, stft_magnitude

N_MELS = 128
AMIN = 1e-10
TOP_DB = 80.0


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3.0
    logstep = np.log(6.4) / 27.0
    with np.errstate(divide="ignore"):
        return np.where(f >= 1000.0, 1000.0 / f_sp + np.log(np.maximum(f, 1e-300) / 1000.0) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3.0
    logstep = np.log(6.4) / 27.0
    return np.where(m >= 1000.0 / f_sp, 1000.0 * np.exp(logstep * (m - 1000.0 / f_sp)), f_sp * m)


def mel_filter_bank(sample_rate, n_fft, n_mels=N_MELS):
    """(n_mels, 1 + n_fft / 2) float64: triangles on the Slaney mel scale, each scaled by 2 / its width in Hz"""
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sample_rate / 2.0), n_mels + 2))
    fft_f = np.linspace(0.0, sample_rate / 2.0, 1 + n_fft // 2)
    lower = (fft_f[None, :] - mel_f[:-2, None]) / (mel_f[1:-1] - mel_f[:-2])[:, None]
    upper = (mel_f[2:, None] - fft_f[None, :]) / (mel_f[2:] - mel_f[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def dct_matrix(n_mfcc, n_mels=N_MELS):
    """(n_mfcc, n_mels): rows of the orthonormal DCT-II"""
    j = np.arange(n_mfcc, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    s = np.where(j == 0, np.sqrt(1.0 / n_mels), np.sqrt(2.0 / n_mels))
    return s * np.cos(np.pi * j * (2.0 * m + 1.0) / (2.0 * n_mels))


def mel_db(audio, sample_rate, n_fft, hop_length, n_mels=N_MELS):
    """(n_mels, T) float64 dB values after the top_db clip, and the clip level"""
    power = stft_magnitude(audio, n_fft, hop_length) ** 2
    mel = mel_filter_bank(sample_rate, n_fft, n_mels) @ power
    db = 10.0 * np.log10(np.maximum(AMIN, mel))
    floor = db.max() - TOP_DB
    return np.maximum(db, floor), floor


def mfcc(audio, sample_rate, n_fft, hop_length, n_mfcc, n_mels=N_MELS):
    """(n_mfcc, 1 + N // hop_length) float64"""
    db, _ = mel_db(audio, sample_rate, n_fft, hop_length, n_mels)
    return dct_matrix(n_mfcc, n_mels) @ db


def clipped_share(audio, sample_rate, n_fft, hop_length, n_mels=N_MELS):
    """share of the dB entries that sit on the top_db clip"""
    db, floor = mel_db(audio, sample_rate, n_fft, hop_length, n_mels)
    return float(np.mean(db <= floor))


def mfcc_float32(audio, sample_rate, n_fft, hop_length, n_mfcc, n_mels=N_MELS):
    """the chain in float32: windowed DFT as a float32 matrix product, float32 mel product, float32 log10, float32 DCT
    (constants built in float64 and rounded once)"""
    y = np.asarray(audio, dtype=np.float32)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    frames = 1 + y.size // hop_length
    idx = hop_length * np.arange(frames)[None, :] + np.arange(n_fft)[:, None]
    x = np.ascontiguousarray(yp[idx])                                            # (n_fft, T) float32
    n = np.arange(n_fft, dtype=np.int64)
    k = np.arange(1 + n_fft // 2, dtype=np.int64)
    phase = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft).astype(np.float64) / n_fft
    win = hann_periodic(n_fft)[None, :]
    re = (win * np.cos(phase)).astype(np.float32) @ x
    im = (-win * np.sin(phase)).astype(np.float32) @ x
    power = re * re + im * im
    mel = mel_filter_bank(sample_rate, n_fft, n_mels).astype(np.float32) @ power
    db = np.float32(10.0) * np.log10(np.maximum(np.float32(AMIN), mel))
    db = np.maximum(db, db.max() - np.float32(TOP_DB))
    out = dct_matrix(n_mfcc, n_mels).astype(np.float32) @ db
    assert out.dtype == np.float32
    return out
