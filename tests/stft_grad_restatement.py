"""Float64 numpy restatement of dL/dx of the multi-resolution STFT loss, written from the definition and not
from the kernels: explicit reflect fold, the windowed DFT as a matrix, torch's three conventions spelt out.

    per resolution r = (n_fft, hop, win_length), X = STFT(x), p = Re^2 + Im^2, x_mag = sqrt(max(p, eps)), y_mag likewise,
    C = B bins frames, R resolutions:
    g    = (1/R) [ w_sc (x_mag - y_mag) / (||y_mag - x_mag||_F ||y_mag||_F)        0 where the first norm is 0
                 + w_log sign(ln x_mag - ln y_mag) / (C x_mag) + w_lin sign(x_mag - y_mag) / C ]         sign(0) = 0
    G    = g X / x_mag where p >= eps, 0 under the clamp                          one-sided bins, no factor 2
    z_t[n] = sum_k D[2k][n] Re G[k,t] + D[2k+1][n] Im G[k,t],   D[2k] = w[n] cos(2 pi k n / n_fft), D[2k+1] = -w[n] sin(..)
    dL/dx[i] = sum of z_t[n] over the padded positions hop t - n_fft/2 + n that reflect onto i; summed over resolutions

Also the broadband pair the log-magnitude checks use next to stft_loss_restatement.signals."""
import functools

import numpy as np

import stft_loss_restatement as sr

signals = sr.signals


@functools.lru_cache(maxsize=None)
def noise_signals(B, N):
    """(x, y) float32 (B, N), read-only: x = 0.1 randn, y = 0.12 randn - every bin of comparable size, so the 1 / x_mag weight
    of the log-magnitude gradient does not single out weak bins next to strong partials"""
    g = np.random.default_rng(7000 * B + N)
    x = (0.1 * g.standard_normal((B, N))).astype(np.float32)
    y = (0.12 * g.standard_normal((B, N))).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _operand(n_fft, win_length):
    """(2 bins, n_fft): rows 2k / 2k+1 = w[n] cos / -w[n] sin"""
    k, n = np.arange(n_fft // 2 + 1)[:, None], np.arange(n_fft)[None, :]
    ph = 2.0 * np.pi * ((k * n) % n_fft) / n_fft
    D = np.empty((2 * (n_fft // 2 + 1), n_fft))
    D[0::2], D[1::2] = np.cos(ph), -np.sin(ph)
    return D * sr.window(n_fft, win_length)


def _frame_index(N, n_fft, hop):
    """(frames, n_fft): the sample of x that column n of frame t reads (reflect, no edge repeat)"""
    p = hop * np.arange(1 + N // hop)[:, None] - n_fft // 2 + np.arange(n_fft)[None, :]
    p = np.abs(p)
    return np.where(p >= N, 2 * (N - 1) - p, p)


def grad(x, y, resolutions=sr.DEFAULT_RESOLUTIONS, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, eps=1e-8):
    """dL/dx, (B, N) float64"""
    x, y = (np.asarray(s, dtype=np.float64).reshape(np.shape(s)[0], np.shape(s)[-1]) for s in (x, y))
    B, N = x.shape
    R = len(resolutions)
    out = np.zeros((B, N))
    for n_fft, hop, win_length in resolutions:
        assert N > n_fft // 2, "reflect padding needs more than n_fft / 2 samples"
        D, idx = _operand(n_fft, win_length), _frame_index(N, n_fft, hop)
        X, Y = x[:, idx] @ D.T, y[:, idx] @ D.T                        # (B, frames, 2 bins), Re / Im interleaved
        p = X[..., 0::2] ** 2 + X[..., 1::2] ** 2
        xm = np.sqrt(np.maximum(p, eps))
        ym = np.sqrt(np.maximum(Y[..., 0::2] ** 2 + Y[..., 1::2] ** 2, eps))
        C = xm.size
        nd, ny = np.sqrt(np.sum((ym - xm) ** 2)), np.sqrt(np.sum(ym ** 2))
        g = w_log_mag * np.sign(np.log(xm) - np.log(ym)) / (C * xm) + w_lin_mag * np.sign(xm - ym) / C
        if nd > 0.0:
            g = g + w_sc * (xm - ym) / (nd * ny)
        g = np.where(p >= eps, g / R, 0.0) / xm                        # the clamp passes nothing below eps
        G = np.empty_like(X)
        G[..., 0::2], G[..., 1::2] = g * X[..., 0::2], g * X[..., 1::2]
        z = G @ D                                                       # (B, frames, n_fft)
        for b in range(B):
            np.add.at(out[b], idx, z[b])                                # overlap-add through the reflect fold
    return out


def row_distance(got, want):
    """largest per-row ||got - want||_2 / ||want||_2"""
    got, want = (np.asarray(a, dtype=np.float64).reshape(np.shape(a)[0], -1) for a in (got, want))
    return float((np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max())


def torch_autograd_grad(x, y, dtype, resolutions=sr.DEFAULT_RESOLUTIONS, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, eps=1e-8):
    """(loss, dL/dx as float64 numpy) by torch's CPU autograd through torch.stft at `dtype`: the expression
    test_cpu_stft_loss.torch_stft_components is built from, with x requiring grad.  float64: the independent yardstick of the
    restatement; float32: what an FFT-based fp32 gradient achieves on the same inputs."""
    import torch

    xt = torch.tensor(np.array(x), dtype=dtype, requires_grad=True)
    yt = torch.tensor(np.array(y), dtype=dtype)
    total = 0.0
    for n_fft, hop, win in resolutions:
        w = torch.hann_window(win, dtype=dtype)

        def mag(s):
            S = torch.stft(s, n_fft, hop, win, window=w, center=True, pad_mode="reflect", normalized=False, onesided=True,
                           return_complex=True)
            return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=eps))
        xm, ym = mag(xt), mag(yt)
        total = total + (w_sc * torch.norm(ym - xm, p="fro") / torch.norm(ym, p="fro")
                         + w_log_mag * (torch.log(xm) - torch.log(ym)).abs().mean() + w_lin_mag * (xm - ym).abs().mean())
    loss = total / len(resolutions)
    loss.backward()
    return float(loss.detach()), xt.grad.double().numpy()
