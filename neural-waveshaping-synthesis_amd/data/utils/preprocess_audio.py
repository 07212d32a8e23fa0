"""The front-end helpers in front of the analysis features on the MI355X (mirror of
neural_waveshaping_synthesis/data/utils/preprocess_audio.py:21-66): integer audio to float32, stereo to mono, level
normalisation, and `resample_audio`, where the reference calls `resampy.resample` and `csrc/resample.hip` runs here
(DESIGN.md 3.10 is the definition; parity with resampy is unpinned).

`resample_audio` accepts a 1-D numpy array like the reference (returns numpy float32), or a (N,) / (B, N) float32 CUDA
tensor (returns a tensor).  No CPU fallback.  The rest of the reference's module (MFCC, segmentation, confidence filtering,
dataset creation) prepares training data and is not part of this package.
"""
from __future__ import annotations

import numpy as np
import torch

from ...engine import binding

_BANK_CACHE: dict = {}


def convert_to_float32_audio(audio: np.ndarray):
    """:21-27: float32 passes through; an integer type is divided by its largest value"""
    if audio.dtype == np.float32:
        return audio
    return (audio / np.iinfo(audio.dtype).max).astype(np.float32)


def make_monophonic(audio: np.ndarray, strategy: str = "keep_left"):
    """:30-58: 1-D passes through; a single channel is unwrapped; (2, N) or (N, 2) is reduced by `strategy`:
    keep_left, keep_right, sum (the mean of the two channels, as in the reference) or diff (left - right)"""
    if audio.ndim == 1:
        return audio
    if audio.ndim != 2:
        raise ValueError(f"audio: expected a 1-D or 2-D array, got {audio.ndim} dimensions")
    if audio.shape[0] == 1:
        return audio[0]
    if audio.shape[1] == 1:
        return audio[:, 0]
    if audio.shape[0] != 2 and audio.shape[1] != 2:
        raise ValueError(f"audio: {audio.shape} is neither mono nor stereo (more than two channels)")
    if audio.shape[1] == 2:            # channel first; a (2, 2) array counts as (N, 2), as in the reference
        audio = audio.T
    if strategy == "keep_left":
        return audio[0]
    if strategy == "keep_right":
        return audio[1]
    if strategy == "sum":
        return np.mean(audio, axis=0)
    if strategy == "diff":
        return audio[0] - audio[1]
    return None                        # the reference falls off its if-chain the same way


def normalise_signal(audio: np.ndarray, factor: float):
    """:61-62"""
    return audio / factor


def _rate(value, name) -> int:
    rate = int(value)
    if rate != value or rate < 1:
        raise ValueError(f"{name} = {value!r}: the resampler takes integral sample rates >= 1")
    return rate


def _bank(sr_in: int, sr_out: int, device) -> torch.Tensor:
    """the weight bank of a pair of rates on `device` (built once on the host)"""
    key = (sr_in, sr_out, str(device))
    b = _BANK_CACHE.get(key)
    if b is None:
        b = binding().resample_bank(sr_in, sr_out).to(device)
        torch.cuda.current_stream(device).synchronize()     # shared by every later caller, whatever its stream
        _BANK_CACHE[key] = b
    return b


def resample_audio(audio, original_sr: float, target_sr: float):
    """:65-66.  (N,) -> ((N L) // M,) with L / M = target_sr / original_sr in lowest terms.  Equal rates still run the filter
    (L = M = 1), as the reference's unconditional call does."""
    sr_in, sr_out = _rate(original_sr, "original_sr"), _rate(target_sr, "target_sr")
    is_numpy = isinstance(audio, np.ndarray)
    if is_numpy:
        if audio.ndim != 1:
            raise ValueError(f"audio: expected a 1-D array, got {audio.shape}")
        x = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).cuda()
    else:
        x = audio
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (1, 2):
        raise RuntimeError("audio: expected a 1-D numpy array or a (N,) / (B, N) float32 CUDA tensor (no CPU fallback)")
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    y = binding().resample(x.contiguous(), _bank(sr_in, sr_out, x.device), sr_in, sr_out)
    if squeeze:
        y = y[0]
    return y.cpu().numpy() if is_numpy else y
