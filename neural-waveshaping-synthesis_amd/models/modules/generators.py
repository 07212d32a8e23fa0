"""Signal generators of the NEWT synthesiser (reference: models/modules/generators.py:11-66).

These classes keep the reference's constructor signatures, buffers and state-dict keys.  Inside
``NeuralWaveshaping.forward`` the DSP runs fused (csrc/exciter_newt.hip: oscillator bank + 101->64 mixer + waveshapers;
csrc/fir_noise.hip: time-varying FIR noise); called on their own the modules run the stand-alone stage kernels
(``oscillator_kernel``; ``fir_from_h_kernel`` + the noise kernel), drawing from the device's default generator exactly
like the reference (``rand_like`` for the phase offsets, ``rand(hop * T - 1)`` for the excitation).
"""
import math
from typing import Callable

import torch
import torch.nn as nn

from ... import ginlite as gin
from . import _standalone as sa


class _FIRNoiseFunction(torch.autograd.Function):
    """FIRNoiseSynth.forward with its transpose attached (csrc/fir_noise_grad.hip): backward runs
    fir_noise_grad and fir_from_h_grad on the excitation the forward used"""

    @staticmethod
    def forward(ctx, H_re, noise, module):
        y = module._forward_detached(H_re.detach(), noise)
        ctx.module = module
        ctx.save_for_backward(noise)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (noise,) = ctx.saved_tensors
        return ctx.module.vjp(grad_out[:, 0], noise), None, None


class _ChannelOffsetFunction(torch.autograd.Function):
    """x + offset[None, :, None]: the add is plumbing, its backward onto the offset is the fixed-order float64 reduction over
    batch and time (sum_batch_time, csrc/fir_noise_grad.hip)"""

    @staticmethod
    def forward(ctx, x, offset):
        return x.detach() + offset.detach()[None, :, None]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        gx = grad_out if ctx.needs_input_grad[0] else None
        go = sa.binding().sum_batch_time(sa.contiguous(grad_out, "grad_out")) if ctx.needs_input_grad[1] else None
        return gx, go


def add_channel_offset(x, offset):
    """(B, C, T) + (C,) per-channel offset -> (B, C, T), differentiable in both: what moves a gradient with respect to the noise
    filter magnitudes H onto the last bias of the MLP that made them (scripts/fit_noise.py)"""
    x = sa.contiguous(x, "x")
    offset = sa._req(offset, "offset", x.shape[1] if x.dim() == 3 else None)
    if x.dim() != 3 or offset.dim() != 1:
        raise RuntimeError(f"add_channel_offset: expected (B, C, T) and (C,), got {tuple(x.shape)} and {tuple(offset.shape)}")
    return _ChannelOffsetFunction.apply(x, offset)


@gin.configurable
class FIRNoiseSynth(nn.Module):
    """Time-varying FIR filtered noise (reference generators.py:11-35).

    ``differentiable`` (a plain attribute, default False): forward only, the result carries no graph and an ``H_re`` that
    requires grad is refused.  Set to True, a forward under grad mode whose ``H_re`` requires grad returns the same bits with a
    ``torch.autograd.Function`` attached that gives dL/dH for the excitation that call used, injected or drawn (the excitation,
    the window and the design matrix get no gradient).  ``vjp`` is the same gradient without autograd."""

    differentiable = False      # also the value of a module unpickled from before the flag existed

    def __init__(self, ir_length: int, hop_length: int, window_fn: Callable = torch.hann_window):
        super().__init__()
        self.ir_length = ir_length
        self.hop_length = hop_length
        self.register_buffer("window", window_fn(ir_length))
        self.differentiable = False
        self._design = {}

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_design"] = {}
        return d

    def _design_matrix(self, dev):
        """window * roll(irfft(.), ir_length / 2) folded into one (256, 132) matrix (nws_fir_design_matrix), per window"""
        win = sa._req(self.window.detach(), "noise_synth.window", sa._lib.FIR_LEN)
        key = (win.data_ptr(), win._version)
        hit = self._design.get(key)
        if hit is None:
            self._design.clear()
            hit = torch.empty(sa._lib.FIR_LEN * sa._lib.FIR_DESIGN_COLS, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                sa.checked(sa._lib.lib().nws_fir_design_matrix(win.data_ptr(), hit.data_ptr(), sa.stream_ptr(dev)),
                           "nws_fir_design_matrix")
            self._design[key] = hit
        return hit

    def _specialised(self):
        return self.ir_length == sa._lib.FIR_LEN and self.hop_length == sa._lib.HOP and self._window_symmetric()

    def _checked_noise(self, noise, T, dev):
        if noise is None:
            noise = torch.rand(self.hop_length * T - 1, device=dev)               # the reference's draw (generators.py:30)
        elif noise.requires_grad:
            raise RuntimeError("FIRNoiseSynth: the excitation gets no gradient (noise requires grad)")
        return sa._req(noise.detach(), "noise", self.hop_length * T - 1)

    def forward(self, H_re, *, noise=None):
        """H_re (B, ir_length/2 + 1, T) real filter magnitudes -> (B, 1, hop * T) filtered noise (generators.py:21-35).
        `noise` injects the excitation draw (hop * T - 1 samples) for parity tests."""
        wants_grad = (self.differentiable and torch.is_grad_enabled() and isinstance(H_re, torch.Tensor) and H_re.requires_grad)
        if not self._specialised():
            if wants_grad:
                raise RuntimeError("FIRNoiseSynth: the runtime-size path (any other ir_length, hop_length or window than 256, 128 "
                                   "and a window symmetric about tap 128) has no gradient; only the specialised kernels have a transpose")
            return self._forward_generic(H_re, noise)
        if wants_grad:
            H = self._checked_H(H_re.detach())                                    # refusals before autograd is involved
            noise = self._checked_noise(noise, H.shape[2], H.device)
            return _FIRNoiseFunction.apply(H_re, noise, self)
        return self._forward_detached(H_re, noise)

    def _checked_H(self, H_re):
        H = sa.contiguous(H_re, "H_re")
        if H.dim() != 3 or H.shape[1] != sa._lib.N_BANDS:
            raise RuntimeError(f"FIRNoiseSynth: expected (B, {sa._lib.N_BANDS}, T), got {tuple(H.shape)}")
        if H.shape[2] < 2:
            raise RuntimeError("need at least 2 frames (reflect padding of the noise STFT, generators.py:31)")
        return H

    def _forward_detached(self, H_re, noise):
        H = self._checked_H(H_re)
        D = self._design_matrix(H.device)
        sa.no_autograd(inputs=(H,))
        noise = self._checked_noise(noise, H.shape[2], H.device)
        b = sa.binding()
        return b.fir_noise(b.fir_from_h(H, D), noise, None, -1).unsqueeze(1)

    def vjp(self, grad_out, noise):
        """dL/dH (B, ir_length/2 + 1, T) of ``forward`` for grad_out = dL/d(out) (B, hop * T) (or (B, 1, hop * T)) and the
        excitation that forward used.  Whatever ``differentiable`` and the grad mode say; autograd is not involved and the result
        carries no graph."""
        if not self._specialised():
            raise RuntimeError("FIRNoiseSynth.vjp: the runtime-size path (any other ir_length, hop_length or window than 256, 128 "
                               "and a window symmetric about tap 128) has no gradient")
        with torch.no_grad():
            g = grad_out.detach()
            if g.dim() == 3 and g.shape[1] == 1:
                g = g[:, 0]
            g = sa.contiguous(g, "grad_out")
            hop = int(self.hop_length)
            if g.dim() != 2 or g.shape[1] % hop or g.shape[1] < 2 * hop:
                raise RuntimeError(f"grad_out: expected (B, {hop} T) with T >= 2, got {tuple(g.shape)}")
            noise = self._checked_noise(noise, g.shape[1] // hop, g.device)
            if noise.device != g.device:
                raise RuntimeError(f"grad_out is on {g.device} but noise is on {noise.device}")
            D = self._design_matrix(g.device)
            b = sa.binding()
            return b.fir_from_h_grad(b.fir_noise_grad(noise, g), D)

    def _window_symmetric(self):
        """the specialised kernels pass half rows of taps (include/nws_hip.h, nws_frame_mlps): needs a window that is symmetric
        about tap L/2 with window[0] == 0, like the reference's periodic Hann"""
        win = self.window
        key = (win.data_ptr(), win._version)
        hit = self.__dict__.get("_win_ok")
        if hit is None or hit[0] != key:
            w = win.detach().float().cpu()
            L = w.numel()
            top = float(w.abs().max())          # symmetric to fp32 rounding (torch.hann_window itself is 1.8e-7 off)
            hit = (key, bool(abs(float(w[0])) <= 1e-7 * top and float((w[1:L // 2] - w[L // 2 + 1:].flip(0)).abs().max()) <= 4e-7 * top))
            self.__dict__["_win_ok"] = hit
        return hit[1]

    def _forward_generic(self, H_re, noise):
        """any even ir_length >= hop_length: runtime-size stage kernels (csrc/generic.hip: g_fir_design_kernel, g_fir_noise_kernel)"""
        L, hop = int(self.ir_length), int(self.hop_length)
        H = sa.contiguous(H_re, "H_re")
        if H.dim() != 3 or H.shape[1] != L // 2 + 1:
            raise RuntimeError(f"FIRNoiseSynth: expected (B, {L // 2 + 1}, T), got {tuple(H.shape)}")
        if L % 2 or L < hop:
            raise RuntimeError(f"FIRNoiseSynth: ir_length {L} must be even and >= hop_length {hop} (torch.istft, generators.py:34)")
        B, _, T = H.shape
        win = sa._req(self.window.detach(), "noise_synth.window", L)
        if noise is None:
            noise = torch.rand(hop * T - 1, device=H.device)                      # the reference's draw (generators.py:30)
        noise = sa._req(noise, "noise", hop * T - 1)
        return sa.call("g_fir_noise", H, win, noise, hop).unsqueeze(1)


@gin.configurable
class HarmonicOscillator(nn.Module):
    def __init__(self, n_harmonics, sample_rate):
        super().__init__()
        self.sample_rate = sample_rate
        self.n_harmonics = n_harmonics
        # same buffers as the reference (generators.py:44-48): k = 1..n as int64, rand_phase = tau
        self.register_buffer("harmonic_axis", torch.arange(1, n_harmonics + 1).view(1, -1, 1))
        self.register_buffer("rand_phase", torch.full((1, n_harmonics, 1), math.tau))

    def forward(self, f0, *, phase_u=None):
        """(B, N) upsampled F0 in Hz -> (B, n_harmonics, N): sin(k * tau * cumsum(f0) / sr + shift_k) * [k f0 < sr / 2]
        (generators.py:58-66; the cumulative sum is accumulated in float64 like torch's CPU cumsum).  N must be a multiple
        of 128.  `phase_u` injects the U[0,1) phase draw for parity tests."""
        f0 = sa.contiguous(f0, "f0")
        if f0.dim() != 2 or f0.shape[1] < 1:
            raise RuntimeError(f"HarmonicOscillator: expected (B, N), got {tuple(f0.shape)}")
        K = int(self.n_harmonics)
        rp = sa._req(self.rand_phase.detach().reshape(-1), "osc.rand_phase", K)
        u = torch.rand_like(self.rand_phase) if phase_u is None else phase_u            # the reference's draw (generators.py:55)
        u = sa._req(u.reshape(-1), "phase_u", K)
        # 101 harmonics on a whole number of hops: the specialised stage kernel; any other harmonic count / length: the
        # runtime-size stage kernels (csrc/generic.hip: g_phase_kernel, g_oscillator_kernel)
        generic = K != sa._lib.N_HARMONICS or f0.shape[1] % sa._lib.HOP
        return sa.call("g_oscillator" if generic else "oscillator", f0, u, rp, float(self.sample_rate))
