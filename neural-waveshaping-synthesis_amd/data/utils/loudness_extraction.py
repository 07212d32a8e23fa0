"""Perceptual-loudness feature on the MI355X (mirror of neural_waveshaping_synthesis/data/utils/loudness_extraction.py).

`extract_perceptual_loudness` keeps the reference's signature, defaults and gin binding names (:41-67), including
`interpolate_fn=linear_interpolation` (a plain call returns loudness at SAMPLE rate, length `audio.size`; the shipped
gin/data/urmp_4second_crepe.gin binds it to None = frame rate); the STFT / dB / mean chain runs in `csrc/loudness.hip`
(one windowed-DFT GEMM on the matrix cores + a dB pass).  Accepts a 1-D numpy array like the reference (returns numpy),
or a (N,) / (B, N) CUDA tensor (returns a tensor per row).  No CPU fallback.

`causal_loudness_frames` / `extract_causal_loudness` are the same feature under the live chain's reference: every
frame against the causal level a `streaming.StreamLoudness` would use, bit for bit, in one call (`csrc/loudness_causal.hip`).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from ... import _lib
from ... import ginlite as gin
from ... import losses
from ...engine import binding
from .upsampling import linear_interpolation


def _dft_operand(n_fft: int, device) -> torch.Tensor:
    """the STFT loss's operand with the hann window as long as the transform; losses.py builds and caches it"""
    return losses._dft_operand(n_fft, n_fft, device)


def loudness_frames(audio: torch.Tensor, n_fft: int, hop_length: int, epsilon: float = 1e-5, top_db: float = 80.0,
                    normalise: bool = True) -> torch.Tensor:
    """(B, N) fp32 CUDA tensor -> (B, 1 + N // hop_length) loudness per frame."""
    if not audio.is_cuda or audio.dtype != torch.float32 or audio.dim() != 2:
        raise RuntimeError("audio: expected a (B, N) float32 CUDA tensor (no CPU fallback)")
    audio = audio.contiguous()
    B, N = audio.shape
    L = _lib.lib()
    nbytes = L.nws_loudness_workspace_bytes(B, N, n_fft, hop_length)
    if nbytes == 0 or N <= n_fft // 2:
        raise RuntimeError(f"unsupported loudness configuration: N={N}, n_fft={n_fft}, hop_length={hop_length} (n_fft: a power "
                           "of two in [64, 2048]; 1 <= hop_length <= n_fft; the 31 * hop_length + n_fft samples one workgroup "
                           "stages must fit 160 KB of LDS, e.g. hop_length <= 1250 at n_fft 2048; N > n_fft / 2)")
    dft = _dft_operand(n_fft, audio.device)
    return binding().loudness(audio, dft, int(n_fft), int(hop_length), float(epsilon), float(top_db), bool(normalise))


def peak_power(audio: torch.Tensor, n_fft: int, hop_length: int) -> torch.Tensor:
    """(B, N) fp32 CUDA tensor -> (B,) fp32 CUDA: the largest power of a bin of the clip's STFT, the reference `loudness_frames`
    normalises by.  As `reference` of a `streaming.StreamLoudness` it makes the stream equal `loudness_frames` of the clip;
    measured on a sound check it is a calibration."""
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda or audio.dtype != torch.float32 or audio.dim() != 2:
        raise RuntimeError("audio: expected a (B, N) float32 CUDA tensor (no CPU fallback)")
    audio = audio.contiguous()
    return binding().loudness_peak_power(audio, _dft_operand(n_fft, audio.device), int(n_fft), int(hop_length))


def release_factor(release_db_per_s: float, hop_length: int, sample_rate: float) -> float:
    """The factor the tracked reference power falls by per frame: 10^(-release_db_per_s hop / (10 sample_rate)),
    computed in float64 and rounded once to the float32 the kernels multiply by.  0 dB/s gives exactly 1: no release."""
    release_db_per_s, sample_rate = float(release_db_per_s), float(sample_rate)
    if not (release_db_per_s >= 0.0 and np.isfinite(release_db_per_s)):
        raise RuntimeError(f"release_db_per_s {release_db_per_s}: expected a finite rate >= 0")
    if not sample_rate > 0.0 or int(hop_length) < 1:
        raise RuntimeError(f"release_factor: sample_rate {sample_rate} and hop_length {hop_length} must be positive")
    rho = float(np.float32(10.0 ** (-release_db_per_s * int(hop_length) / (10.0 * sample_rate))))
    if not 0.0 < rho <= 1.0:
        raise RuntimeError(f"release_db_per_s {release_db_per_s}: the factor per frame underflows float32")
    return rho


def _floor_powers(value, B: int, device, name: str = "floor_power") -> torch.Tensor:
    """None (0), a power or a (B,) tensor of powers -> (B,) fp32 on `device`; checked here (this reads a tensor back)"""
    if isinstance(value, torch.Tensor):
        p = value.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        if p.numel() != B:
            raise RuntimeError(f"{name}: expected ({B},) powers, got {tuple(value.shape)}")
    else:
        p = torch.full((B,), 0.0 if value is None else float(value), dtype=torch.float32, device=device)
    if not bool((torch.isfinite(p) & (p >= 0)).all()):
        raise RuntimeError(f"{name}: powers must be finite and >= 0")
    return p


def causal_loudness_frames(audio: torch.Tensor, n_fft: int, hop_length: int, lag: int = 8, release_db_per_s: float = 0.0,
                           sample_rate: float = 16000, floor_power=None, epsilon: float = 1e-5, top_db: float = 80.0,
                           normalise: bool = True):
    """(B, N) fp32 CUDA tensor -> (loudness, reference_power, frame_peak_power), (B, 1 + N // hop_length) each: what a
    `streaming.StreamLoudness(reference="running", lag=lag, release_db_per_s=..., floor_power=...)` releases over the clip and
    its flush, bit for bit and whatever the chunking, in one call (`csrc/loudness_causal.hip`).  A dataset built
    with it measures every frame against the reference the live chain uses instead of the peak of the whole clip."""
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda or audio.dtype != torch.float32 or audio.dim() != 2:
        raise RuntimeError("audio: expected a (B, N) float32 CUDA tensor (no CPU fallback)")
    audio = audio.contiguous()
    rho = release_factor(release_db_per_s, hop_length, sample_rate)
    floors = _floor_powers(floor_power, audio.shape[0], audio.device)
    return tuple(binding().loudness_causal(audio, _dft_operand(n_fft, audio.device), int(n_fft), int(hop_length), int(lag), rho, floors,
                                           True, float(epsilon), float(top_db), bool(normalise)))


def _frames_to_output(out, x, n_fft, hop_length, interpolate_fn, normalise, squeeze, is_numpy):
    """the frames of (B, T) `out` (not normalised if interpolate_fn) -> what the reference's extractor returns"""
    if interpolate_fn:
        rows = [interpolate_fn(r, n_fft, hop_length, original_length=x.shape[1]) for r in out.cpu().numpy().astype(np.float64)]
        res = np.stack(rows)
        if normalise:
            res = (res + 80) / 80
        res = res[0] if squeeze else res
        return res if is_numpy else torch.as_tensor(res)
    if squeeze:
        out = out[0]
    return out.cpu().numpy() if is_numpy else out


@gin.configurable
def extract_causal_loudness(audio, sample_rate: float = 16000, n_fft: int = 2048, hop_length: int = 512, window: str = "hann",
                            epsilon: float = 1e-5, interpolate_fn: Optional[Callable] = linear_interpolation,
                            normalise: bool = True, lag: int = 8, release_db_per_s: float = 0.0, floor_power=None):
    """`extract_perceptual_loudness` under the live chain's reference: every frame against the causal level of DESIGN.md 3.26
    (`causal_loudness_frames`) instead of the peak of the whole clip.  The first eight parameters are the offline extractor's, so
    a gin file binds it as `preprocess_audio.loudness_extractor` in its place (gin/data/urmp_4second_pyin_live.gin)."""
    if window != "hann":
        raise RuntimeError("only the reference's hann window is implemented")
    is_numpy = isinstance(audio, np.ndarray)
    x = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).cuda() if is_numpy else audio
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    out = causal_loudness_frames(x, n_fft, hop_length, lag, release_db_per_s, sample_rate, floor_power, epsilon, 80.0,
                                 normalise=normalise and not interpolate_fn)[0]
    return _frames_to_output(out, x, n_fft, hop_length, interpolate_fn, normalise, squeeze, is_numpy)


@gin.configurable
def extract_perceptual_loudness(audio, sample_rate: float = 16000, n_fft: int = 2048, hop_length: int = 512,
                                window: str = "hann", epsilon: float = 1e-5,
                                interpolate_fn: Optional[Callable] = linear_interpolation, normalise: bool = True):
    """loudness_extraction.py:41-67.  (sample_rate only fed the A-weighting, which the reference computes and then does not
    apply, :38.)  interpolate_fn, if given, is called exactly like the reference calls it, on the host."""
    if window != "hann":
        raise RuntimeError("only the reference's hann window is implemented")
    is_numpy = isinstance(audio, np.ndarray)
    x = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).cuda() if is_numpy else audio
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    # normalisation is applied after the optional interpolation, as in the reference (both are affine, order kept anyway)
    out = loudness_frames(x, n_fft, hop_length, epsilon, 80.0, normalise=normalise and not interpolate_fn)
    return _frames_to_output(out, x, n_fft, hop_length, interpolate_fn, normalise, squeeze, is_numpy)
