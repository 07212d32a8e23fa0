"""Float64 numpy restatement of the learned reverb's transpose, written from the definition and not from the
kernels.  Reference forward (models/modules/shaping.py:161-173), Lc = max(N, ir_len + 1), h = [0, ir, 0 ...] of length Lc,
x_ and g_ = x and g = dL/dy zero-padded from N to Lc and read as Lc-periodic:

    y[b, n]    = x[b, n] + sum_m h[m] x_[b, (n - m) mod Lc]                     n < N
    dx[b, i]   = g[b, i] + sum_m h[m] g_[b, (i + m) mod Lc]                     i < N            circular correlation with h
    dir[j - 1] = sum_b sum_{n < N} g[b, n] x_[b, (n - j) mod Lc]                j = 1 .. ir_len  summed over the batch

Two forms of each: through numpy's complex FFT of length Lc (any size), and with every index written out, O(N ir_len), for tiny
sizes.  `initial_zero` is a buffer and gets no gradient.  Also the deterministic inputs of the reverb-gradient tests."""
import functools

import numpy as np


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def _padded(a, Lc):
    out = np.zeros(a.shape[:-1] + (Lc,))
    out[..., :a.shape[-1]] = a
    return out


def circular_length(N, ir_len):
    return max(N, ir_len + 1)


# ---- FFT form ------------------------------------------------------------------------------------------------------------------
def forward(x, ir):
    """y (B, N) float64"""
    x, ir = _f64(x, np.reshape(ir, -1))
    N, Lc = x.shape[-1], circular_length(x.shape[-1], ir.size)
    h = _padded(np.concatenate(([0.0], ir)), Lc)
    wet = np.fft.ifft(np.fft.fft(_padded(x, Lc)) * np.fft.fft(h)).real
    return x + wet[..., :N]


def grad_x(g, ir):
    """dL/dx (B, N) float64"""
    g, ir = _f64(g, np.reshape(ir, -1))
    N, Lc = g.shape[-1], circular_length(g.shape[-1], ir.size)
    h = _padded(np.concatenate(([0.0], ir)), Lc)
    wet = np.fft.ifft(np.fft.fft(_padded(g, Lc)) * np.conj(np.fft.fft(h))).real
    return g + wet[..., :N]


def grad_ir(x, g, ir_len):
    """dL/d(ir) (ir_len,) float64, summed over the batch"""
    x, g = _f64(x, g)
    Lc = circular_length(x.shape[-1], ir_len)
    c = np.fft.ifft(np.sum(np.conj(np.fft.fft(_padded(x, Lc))) * np.fft.fft(_padded(g, Lc)), axis=0)).real
    return c[1:ir_len + 1]


# ---- every index written out (tiny sizes) -------------------------------------------------------------------------------------------
def forward_explicit(x, ir):
    x, ir = _f64(x, np.reshape(ir, -1))
    (B, N), Lc = x.shape, circular_length(x.shape[-1], ir.size)
    x_ = _padded(x, Lc)
    y = x.copy()
    for n in range(N):
        for m in range(1, ir.size + 1):
            y[:, n] += ir[m - 1] * x_[:, (n - m) % Lc]
    return y


def grad_x_explicit(g, ir):
    g, ir = _f64(g, np.reshape(ir, -1))
    (B, N), Lc = g.shape, circular_length(g.shape[-1], ir.size)
    g_ = _padded(g, Lc)
    dx = g.copy()
    for i in range(N):
        for m in range(1, ir.size + 1):
            dx[:, i] += ir[m - 1] * g_[:, (i + m) % Lc]
    return dx


def grad_ir_explicit(x, g, ir_len):
    x, g = _f64(x, g)
    (B, N), Lc = x.shape, circular_length(x.shape[-1], ir_len)
    x_ = _padded(x, Lc)
    d = np.zeros(ir_len)
    for j in range(1, ir_len + 1):
        for n in range(N):
            d[j - 1] += float(np.dot(g[:, n], x_[:, (n - j) % Lc]))
    return d


# ---- distances -----------------------------------------------------------------------------------------------------------------
def rel_l2(got, want):
    """||got - want||_2 / ||want||_2 over all elements: also the RMS of the difference over the RMS of the reference"""
    got, want = _f64(got, want)
    return float(np.linalg.norm(got.ravel() - want.ravel()) / np.linalg.norm(want.ravel()))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(B, N, ir_len):
    """(x, g, ir) float32, read-only: x (B, N) and g (B, N) seeded normal; ir[j] = 0.2 exp(-6 j / ir_len) normal, (1, ir_len),
    so that the wet path weighs about as much as the dry one (a checkpoint's IR is too weak to show an error in it)"""
    rng = np.random.default_rng(1000003 * B + 31 * N + ir_len)
    x = rng.standard_normal((B, N)).astype(np.float32)
    g = rng.standard_normal((B, N)).astype(np.float32)
    ir = (0.2 * np.exp(-6.0 * np.arange(ir_len) / ir_len) * rng.standard_normal(ir_len)).astype(np.float32).reshape(1, ir_len)
    for a in (x, g, ir):
        a.setflags(write=False)
    return x, g, ir


def torch_autograd_grads(x, g, ir, dtype):
    """(dx (B, N), dir (ir_len,)) as float64 numpy by torch's CPU autograd at `dtype` through the reference expression
    (models/modules/shaping.py:161-173: cat, pad, rfft x rfft, irfft, slice) of L = sum(y g).  float64: the independent check
    of the formulas above; float32: what an FFT-based fp32 gradient achieves on the same inputs."""
    import torch
    import torch.nn.functional as F

    xt = torch.tensor(np.array(x), dtype=dtype, requires_grad=True)
    irt = torch.tensor(np.array(ir), dtype=dtype).reshape(1, -1).requires_grad_()
    gt = torch.tensor(np.array(g), dtype=dtype)
    ir_ = torch.cat((torch.zeros(1, 1, dtype=dtype), irt), dim=-1)
    if xt.shape[-1] > ir_.shape[-1]:
        ir_ = F.pad(ir_, (0, xt.shape[-1] - ir_.shape[-1]))
        x_ = xt
    else:
        x_ = F.pad(xt, (0, ir_.shape[-1] - xt.shape[-1]))
    y = xt + torch.fft.irfft(torch.fft.rfft(x_) * torch.fft.rfft(ir_))[..., : xt.shape[-1]]
    (y * gt).sum().backward()
    return xt.grad.double().numpy(), irt.grad.double().numpy().reshape(-1)
