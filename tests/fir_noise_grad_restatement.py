"""Float64 numpy restatement of the noise branch's backward, written from the definition and not from the
kernels.  Reference forward (models/modules/generators.py:21-35), L = 256, hop = 128, T frames, N = 128 T, excitation u of
M = N - 1 samples, D the (256, 129) design matrix (window * roll(irfft(.), 128)):

    h_t[n]   = sum_k D[n][k] H[k, t]                                        the 256 taps of frame t
    x_t[n]   = u[refl(128 (t - 1) + n)]       refl(i) = -i (i < 0), 2 (M - 1) - i (i > M - 1)
    y_t[n]   = sum_m h_t[m] x_t[(n - m) mod 256]
    out[j]   = (1 / c[j]) sum_t y_t[j - 128 t]      j < N, c[j] = 1 (j < 128) else 2; the upper half of frame T - 1 is cropped

and for g = dL/d(out), g^[j] = g[j] / c[j] (j < N), 0 (N <= j < N + 128):

    dh_t[m]  = sum_{n<256} g^[128 t + n] x_t[(n - m) mod 256]
    du_t[d]  = dh_t[128 + d] + dh_t[128 - d] (d = 1 .. 127), du_t[0] = dh_t[128]     gradient of the stored half row
    dH[k, t] = sum_{d<128} D[128 + d][k] du_t[d]     ( = sum_{n<256} D[n][k] dh_t[n] for a window symmetric about tap 128, w[0] = 0 )

dh is written twice: with every index spelled out, and through 256-point FFTs (dh_t = IDFT(conj(X_t) G_t)).  Also the
deterministic inputs of the tests, the distance they use, and torch's autograd through the reference expression."""
import functools

import numpy as np

L, HOP, BANDS = 256, 128, 129


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def hann_periodic(n=L):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def design_matrix(window=None):
    """D (256, 129) float64: h = D @ H is window * roll(irfft(H), 128) of a real H (generators.py:22-27)"""
    w = hann_periodic() if window is None else np.asarray(window, dtype=np.float64)
    n, k = np.arange(L)[:, None], np.arange(BANDS)[None, :]
    ck = np.where((k == 0) | (k == L // 2), 1.0, 2.0)
    return w[:, None] * ck * np.cos(2.0 * np.pi * k * (n - L // 2) / L) / L


def refl(i, M):
    i = -i if i < 0 else i
    return 2 * (M - 1) - i if i > M - 1 else i


def noise_frames(u, T):
    """x (T, 256): x_t[n] = u[refl(128 (t - 1) + n)]"""
    (u,) = _f64(u)
    assert u.shape == (HOP * T - 1,)
    return np.array([[u[refl(HOP * (t - 1) + n, u.size)] for n in range(L)] for t in range(T)])


def g_hat(g):
    """(B, N + 128): g / c, and zeros over the cropped half of the last frame"""
    (g,) = _f64(g)
    out = np.zeros((g.shape[0], g.shape[1] + HOP))
    out[:, :g.shape[1]] = g * 0.5
    out[:, :HOP] = g[:, :HOP]
    return out


# ---- forward (for the transpose identities and the optimisation targets) -----------------------------------------------------------
def taps(H, window=None):
    """h (B, T, 256) from H (B, 129, T)"""
    (H,) = _f64(H)
    return np.einsum("nk,bkt->btn", design_matrix(window), H)


def forward_from_taps(h, u):
    """out (B, N) from full tap rows h (B, T, 256)"""
    (h,) = _f64(h)
    B, T, _ = h.shape
    x = noise_frames(u, T)
    y = np.fft.ifft(np.fft.fft(h, axis=-1) * np.fft.fft(x, axis=-1)[None], axis=-1).real
    out = np.zeros((B, HOP * (T + 1)))
    for t in range(T):
        out[:, HOP * t: HOP * t + L] += y[:, t]
    out[:, HOP:] *= 0.5
    return out[:, : HOP * T]


def full_rows(half):
    """h (B, T, 256) from the stored half rows (B, T, 128): h[128 + d] = h[128 - d] = half[d], h[0] = 0"""
    (half,) = _f64(half)
    h = np.zeros(half.shape[:-1] + (L,))
    h[..., HOP:] = half
    h[..., 1:HOP] = half[..., :0:-1]
    return h


def forward(H, u, window=None):
    return forward_from_taps(taps(H, window), u)


# ---- dh: every index spelled out ------------------------------------------------------------------------------------------------------
def grad_taps_explicit(u, g):
    """dh (B, T, 256)"""
    gh = g_hat(g)
    B, T = gh.shape[0], gh.shape[1] // HOP - 1
    x = noise_frames(u, T)
    dh = np.zeros((B, T, L))
    m = np.arange(L)
    for t in range(T):
        for n in range(L):
            dh[:, t, m] += gh[:, HOP * t + n, None] * x[t, (n - m) % L][None, :]
    return dh


# ---- dh: through 256-point FFTs ---------------------------------------------------------------------------------------------------------
def grad_taps_fft(u, g):
    """dh (B, T, 256) = IDFT(conj(X_t) G_t)"""
    gh = g_hat(g)
    B, T = gh.shape[0], gh.shape[1] // HOP - 1
    X = np.fft.fft(noise_frames(u, T), axis=-1)
    G = np.fft.fft(np.stack([gh[:, HOP * t: HOP * t + L] for t in range(T)], axis=1), axis=-1)
    return np.fft.ifft(np.conj(X)[None] * G, axis=-1).real


def fold(dh):
    """du (B, T, 128): the gradient of the stored half row"""
    (dh,) = _f64(dh)
    du = dh[..., HOP:].copy()
    for d in range(1, HOP):
        du[..., d] += dh[..., HOP - d]
    return du


def grad_H_from_half(du, window=None):
    """dH (B, 129, T) = D[128:]^T du"""
    (du,) = _f64(du)
    return np.einsum("dk,btd->bkt", design_matrix(window)[HOP:], du)


def grad_H_from_full(dh, window=None):
    """dH (B, 129, T) = D^T dh: the transpose of h = D H with no symmetry assumed"""
    (dh,) = _f64(dh)
    return np.einsum("nk,btn->bkt", design_matrix(window), dh)


def grad_fir(u, g):
    return fold(grad_taps_fft(u, g))


def grad_H(u, g, window=None):
    return grad_H_from_half(grad_fir(u, g), window)


# ---- distances -----------------------------------------------------------------------------------------------------------------------
def rel_l2(got, want):
    """||got - want||_2 / ||want||_2 over all elements"""
    got, want = _f64(got, want)
    return float(np.linalg.norm(got.ravel() - want.ravel()) / np.linalg.norm(want.ravel()))


def worst_row(got, want):
    """the largest per-row relative L2 (rows = the leading axis: utterances)"""
    return max(rel_l2(a, b) for a, b in zip(np.asarray(got), np.asarray(want)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(B, T):
    """(H (B, 129, T), u (128 T - 1), g (B, 128 T)) float32, read-only: H = 0.5 + 0.3 normal, u uniform in [0, 1) (mean 0.5: every
    correlation carries a large common term), g normal"""
    rng = np.random.default_rng(7919 * B + T)
    H = (0.5 + 0.3 * rng.standard_normal((B, BANDS, T))).astype(np.float32)
    u = rng.random(HOP * T - 1).astype(np.float32)
    g = rng.standard_normal((B, HOP * T)).astype(np.float32)
    for a in (H, u, g):
        a.setflags(write=False)
    return H, u, g


def torch_reference(H_re, noise, window):
    """the reference expression (generators.py:21-35) on torch tensors with the draw injected -> (out (B, N), h (B, T, 256))"""
    import torch

    h = torch.fft.irfft(torch.complex(H_re, torch.zeros_like(H_re)).transpose(1, 2))
    h = h.roll(L // 2, -1)
    h = h * window.view(1, 1, -1)
    if h.requires_grad:
        h.retain_grad()
    Hf = torch.fft.rfft(h)
    X = torch.stft(noise, L, HOP, return_complex=True).unsqueeze(0)
    y = torch.istft(X * Hf.transpose(1, 2), L, HOP, center=False)
    return y[:, : H_re.shape[-1] * HOP], h


def torch_autograd_grads(H, noise, g, dtype):
    """(du (B, T, 128), dH (B, 129, T)) as float64 numpy by torch's CPU autograd at `dtype` through the reference expression of
    L = sum(out g); du is the fold of autograd's dL/dh.  float64: the independent check of the formulas above; float32: what an
    FFT-based fp32 gradient achieves on the same inputs."""
    import torch

    Ht = torch.tensor(np.array(H), dtype=dtype, requires_grad=True)
    out, h = torch_reference(Ht, torch.tensor(np.array(noise), dtype=dtype), torch.hann_window(L, dtype=dtype))
    (out * torch.tensor(np.array(g), dtype=dtype)).sum().backward()
    return fold(h.grad.double().numpy()), Ht.grad.double().numpy()
