"""Float64 numpy restatement of the multi-resolution STFT loss, written from the definition and not from the
kernel: explicit reflect padding, the hann window of win_length centred in n_fft, numpy's rfft, the clamp on the power.

    x: the reconstruction, y: the target, (B, N);  resolution r = (n_fft, hop, win_length)
    mag   = sqrt(max(|STFT|^2, eps))                         (B, bins, frames), frames = 1 + N // hop
    sc_r  = ||y_mag - x_mag||_F / ||y_mag||_F                over the whole array, normalised by the TARGET
    log_r = mean |ln x_mag - ln y_mag|,   lin_r = mean |x_mag - y_mag|
    loss  = sum_r (w_sc sc_r + w_log_mag log_r + w_lin_mag lin_r) / R

Also the signals the tests share (decaying sines + noise, as the issue that asked for the loss describes them)."""
import functools

import numpy as np

DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
SHAPES = ((1, 1100), (3, 4000), (2, 16000))


def window(n_fft, win_length):
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)     # periodic hann
    return w


def magnitude(s, n_fft, hop, win_length, eps=1e-8):
    """(B, N) -> (B, n_fft // 2 + 1, 1 + N // hop) float64"""
    s = np.asarray(s, dtype=np.float64)
    s = s.reshape(s.shape[0], s.shape[-1])
    N = s.shape[1]
    half = n_fft // 2
    assert N > half, "reflect padding needs more than n_fft / 2 samples"
    i = np.abs(np.arange(-half, N + half))                      # reflect, no edge repeat: -1 -> 1, N -> N - 2
    padded = s[:, np.where(i >= N, 2 * (N - 1) - i, i)]
    frames = 1 + N // hop
    idx = hop * np.arange(frames)[:, None] + np.arange(n_fft)[None, :]          # frame t covers [hop t - half, hop t + half)
    S = np.fft.rfft(padded[:, idx] * window(n_fft, win_length), axis=-1)        # (B, frames, bins)
    power = S.real ** 2 + S.imag ** 2
    return np.sqrt(np.maximum(power, eps)).transpose(0, 2, 1)


def components(x, y, resolutions=DEFAULT_RESOLUTIONS, eps=1e-8):
    """(R, 3): sc_r, log_r, lin_r"""
    out = []
    for n_fft, hop, win_length in resolutions:
        xm, ym = magnitude(x, n_fft, hop, win_length, eps), magnitude(y, n_fft, hop, win_length, eps)
        out.append([np.sqrt(np.sum((ym - xm) ** 2)) / np.sqrt(np.sum(ym ** 2)), np.mean(np.abs(np.log(xm) - np.log(ym))),
                    np.mean(np.abs(xm - ym))])
    return np.array(out, dtype=np.float64)


def loss(x, y, resolutions=DEFAULT_RESOLUTIONS, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, eps=1e-8):
    c = components(x, y, resolutions, eps)
    return float(np.sum(c @ np.array([w_sc, w_log_mag, w_lin_mag])) / len(resolutions))


@functools.lru_cache(maxsize=None)
def signals(B, N):
    """(x, y) float32 (B, N), read-only: decaying sines at 220 (b + 1) Hz over a noise floor that keeps every bin far above the
    eps clamp; x differs from y in level, phase, decay and noise"""
    g = np.random.default_rng(1000 * B + N)
    t = np.arange(N) / 16000.0
    y = np.stack([0.3 * np.sin(2 * np.pi * 220.0 * (b + 1) * t) * np.linspace(1.0, 0.2, N) + 0.01 * g.standard_normal(N)
                  for b in range(B)])
    x = np.stack([0.25 * np.sin(2 * np.pi * 220.0 * (b + 1) * t + 0.3) * np.linspace(1.0, 0.3, N) + 0.02 * g.standard_normal(N)
                  for b in range(B)])
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(B, N):
    """(loss, components) of signals(B, N) at the default resolutions, computed once"""
    x, y = signals(B, N)
    c = components(x, y)
    c.setflags(write=False)
    return float(np.sum(c[:, 0] + c[:, 1]) / len(c)), c
