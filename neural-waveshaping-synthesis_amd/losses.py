"""Multi-resolution STFT loss on the MI355X: the number the reference logs as ``val/loss`` and ``test/loss``.

``STFTLoss`` and ``MultiResolutionSTFTLoss`` carry the constructor names and defaults of ``auraloss.freq`` (0.2.1, the
version the reference pins) for the subset the reference uses: hann window, spectral convergence + log magnitude
(+ linear magnitude), mean reduction.  ``forward(x, y)`` - x the reconstruction, y the target, ``(B, N)`` or ``(B, 1, N)``
float32 CUDA tensors - is one call of ``csrc/stft_loss.hip``: one fused kernel per resolution and a finalise kernel, no
spectrogram in memory, no host synchronisation, equal bits for equal inputs.  DESIGN.md 3.12 is the definition; parity with
auraloss itself is unpinned (it is not a dependency of this package).

By default forward only: tensors that require grad are refused under grad mode.  ``differentiable=True`` attaches the gradient
with respect to the reconstruction x (``csrc/stft_grad.hip``) as a ``torch.autograd.Function``, and
``loss_and_grad(x, y)`` returns the loss and dL/dx without touching autograd.  The target y never gets a gradient, and there
is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .engine import binding

_DFT_CACHE: dict = {}

_REFUSED = "this package implements the subset of auraloss.freq the reference uses (DESIGN.md 3.12)"


def _dft_operand(n_fft: int, win_length: int, device) -> torch.Tensor:
    """window-folded DFT operand of a resolution on `device` (built there once)"""
    key = (n_fft, win_length, str(device))
    t = _DFT_CACHE.get(key)
    if t is None:
        with torch.cuda.device(device):
            t = binding().stft_loss_dft(n_fft, win_length)
            torch.cuda.current_stream(device).synchronize()     # shared by every later caller, whatever its stream
        _DFT_CACHE[key] = t
    return t


class _STFTLossFunction(torch.autograd.Function):
    """loss = module(x, y) with dL/dx from the HIP kernels; y and the module get no gradient"""

    @staticmethod
    def forward(ctx, x, y, module):
        ctx.module = module
        ctx.save_for_backward(x, y)
        return module._call(x, y)[0]          # grad mode is off in here

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        x, y = ctx.saved_tensors
        return ctx.module._grad(x, y) * grad_output, None, None


def _check_variant(window, w_phs, kwargs):
    if window != "hann_window":
        raise ValueError(f"window = {window!r}: only 'hann_window' is implemented; {_REFUSED}")
    if float(w_phs) != 0.0:
        raise ValueError(f"w_phs = {w_phs}: the phase term is not implemented; {_REFUSED}")
    refused = {"sample_rate": None, "scale": None, "n_bins": None, "scale_invariance": False, "reduction": "mean",
               "device": None, "output": "loss"}
    for k, v in kwargs.items():
        if k not in refused:
            raise TypeError(f"unexpected keyword argument {k!r}")
        if v != refused[k]:
            raise ValueError(f"{k} = {v!r}: only {refused[k]!r} is implemented; {_REFUSED}")


class MultiResolutionSTFTLoss(nn.Module):
    """auraloss.freq.MultiResolutionSTFTLoss: the mean over resolutions of w_sc sc + w_log_mag log + w_lin_mag lin."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240),
                 window: str = "hann_window", w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0,
                 w_phs: float = 0.0, eps: float = 1e-8, *, differentiable: bool = False, **kwargs):
        super().__init__()
        _check_variant(window, w_phs, kwargs)
        self.differentiable = bool(differentiable)
        fft_sizes, hop_sizes, win_lengths = ([int(v) for v in seq] for seq in (fft_sizes, hop_sizes, win_lengths))
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
            raise ValueError(f"fft_sizes, hop_sizes and win_lengths must have one length, got {len(fft_sizes)}, {len(hop_sizes)}, "
                             f"{len(win_lengths)}")
        if not 1 <= len(fft_sizes) <= 8:
            raise ValueError(f"1 to 8 resolutions, got {len(fft_sizes)}")
        for n, h, w in zip(fft_sizes, hop_sizes, win_lengths):
            if n < 64 or n > 2048 or n & (n - 1):
                raise ValueError(f"fft_size = {n}: the kernel takes a power of two in [64, 2048]")
            if not 1 <= w <= n:
                raise ValueError(f"win_length = {w}: must lie in [1, fft_size = {n}]")
            if h < 1:
                raise ValueError(f"hop_size = {h}: must be at least 1")
        if not float(eps) > 0.0:
            raise ValueError(f"eps = {eps}: must be positive")
        self.fft_sizes, self.hop_sizes, self.win_lengths = fft_sizes, hop_sizes, win_lengths
        self.window = window
        self.w_sc, self.w_log_mag, self.w_lin_mag, self.w_phs = float(w_sc), float(w_log_mag), float(w_lin_mag), 0.0
        self.eps = float(eps)

    def _prepare(self, x: torch.Tensor, y: torch.Tensor):
        """the checks every entry shares -> x, y as contiguous (B, N) and the operands of the resolutions"""
        for name, t in (("x", x), ("y", y)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name}: expected a tensor")
            if not t.is_cuda:
                raise RuntimeError(f"{name} lives on {t.device}: the STFT loss only runs as HIP kernels on an AMD GPU (there is no "
                                   "CPU fallback)")
            if t.dtype != torch.float32:
                raise TypeError(f"{name}: expected float32, got {t.dtype}")
            if torch.is_grad_enabled() and t.requires_grad:
                if self.differentiable and name == "y":
                    raise RuntimeError("y requires grad: the target gets no gradient from the STFT loss (only the reconstruction x "
                                       "does). Detach it.")
                raise RuntimeError(f"{name} requires grad: the STFT loss kernels are forward-only (no backward pass in this package). "
                                   "Detach it or call under torch.no_grad().")
        if x.shape != y.shape:
            raise RuntimeError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have the same shape")
        if x.device != y.device:
            raise RuntimeError(f"x is on {x.device} but y is on {y.device}")
        if not (x.dim() == 2 or (x.dim() == 3 and x.shape[1] == 1)):
            raise RuntimeError(f"expected (B, N) or (B, 1, N), got {tuple(x.shape)}")
        x = x.reshape(x.shape[0], x.shape[-1]).contiguous()
        y = y.reshape(y.shape[0], y.shape[-1]).contiguous()
        dfts = [_dft_operand(n, w, x.device) for n, w in zip(self.fft_sizes, self.win_lengths)]
        return x, y, dfts

    def _call(self, x: torch.Tensor, y: torch.Tensor):
        x, y, dfts = self._prepare(x, y)
        return binding().stft_loss(x, y, dfts, self.fft_sizes, self.hop_sizes, self.win_lengths, self.w_sc, self.w_log_mag,
                                   self.w_lin_mag, self.eps)

    def _grad(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """dL/dx in the shape of x; outside autograd"""
        with torch.no_grad():
            x2, y2, dfts = self._prepare(x, y)
            g = binding().stft_loss_grad(x2, y2, dfts, self.fft_sizes, self.hop_sizes, self.win_lengths, self.w_sc, self.w_log_mag,
                                         self.w_lin_mag, self.eps)
        return g.reshape(x.shape)

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """0-dim tensor on the inputs' device.  Not symmetric: the spectral convergence is normalised by the target y.
        With ``differentiable=True`` and an x that requires grad, the result carries dL/dx (same loss bits)."""
        if self.differentiable and torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
            self._prepare(x.detach(), y)                # refusals (a y that requires grad among them) before autograd is involved
            return _STFTLossFunction.apply(x, y, self)
        return self._call(x, y)[0]

    def loss_and_grad(self, x: torch.Tensor, y: torch.Tensor):
        """(loss, dL/dx): the 0-dim loss of ``forward`` and its gradient in the shape of x, whatever ``differentiable`` and the
        grad mode say; autograd is not involved and the results carry no graph"""
        with torch.no_grad():
            return self._call(x, y)[0], self._grad(x, y)

    def components(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """(R, 3): spectral convergence, log-magnitude and linear-magnitude distance of every resolution, unweighted; forward only"""
        return self._call(x, y)[1]


class STFTLoss(MultiResolutionSTFTLoss):
    """auraloss.freq.STFTLoss: one resolution."""

    def __init__(self, fft_size: int = 1024, hop_size: int = 256, win_length: int = 1024, window: str = "hann_window",
                 w_sc: float = 1.0, w_log_mag: float = 1.0, w_lin_mag: float = 0.0, w_phs: float = 0.0, eps: float = 1e-8,
                 *, differentiable: bool = False, **kwargs):
        super().__init__([fft_size], [hop_size], [win_length], window, w_sc, w_log_mag, w_lin_mag, w_phs, eps,
                         differentiable=differentiable, **kwargs)
        self.fft_size, self.hop_size, self.win_length = self.fft_sizes[0], self.hop_sizes[0], self.win_lengths[0]
