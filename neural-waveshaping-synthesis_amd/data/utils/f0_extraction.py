"""F0 extraction on the MI355X (mirror of neural_waveshaping_synthesis/data/utils/f0_extraction.py).

`extract_f0_with_pyin` keeps the reference's signature, defaults and gin binding names (:60-92), including
`interpolate_fn=linear_interpolation` (a plain call returns F0 and voiced probability at SAMPLE rate).  Where the reference
calls `librosa.pyin`, the three stages of `csrc/pyin.hip` run: squared-difference YIN with cumulative-mean normalisation,
the threshold-prior observation stage, the HMM decode (DESIGN.md 3.9 is the definition; parity with librosa is unpinned).
Accepts a 1-D numpy array like the reference (returns numpy float64), or a (N,) / (B, N) float32 CUDA tensor (returns
tensors).  No CPU fallback.

`extract_f0_with_crepe` exists so that a gin file binding it parses; CREPE needs torchcrepe and its weights and is not
available here.
"""
from __future__ import annotations

from typing import Callable, Optional, Union

import numpy as np
import torch

from ... import ginlite as gin
from ...engine import binding
from .upsampling import linear_interpolation

CREPE_WINDOW_LENGTH = 1024

_TABLE_CACHE: dict = {}


def _config(sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length):
    return float(sample_rate), float(minimum_frequency), float(maximum_frequency), int(frame_length), int(hop_length)


def _table(cfg, device) -> torch.Tensor:
    """the fp64 constants of a configuration on `device` (built once on the host)"""
    key = (cfg, str(device))
    t = _TABLE_CACHE.get(key)
    if t is None:
        t = binding().pyin_table(*cfg).to(device)
        torch.cuda.current_stream(device).synchronize()     # shared by every later caller, whatever its stream
        _TABLE_CACHE[key] = t
    return t


def _audio(audio: torch.Tensor, frame_length: int) -> torch.Tensor:
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda or audio.dtype != torch.float32 or audio.dim() != 2:
        raise RuntimeError("audio: expected a (B, N) float32 CUDA tensor (no CPU fallback)")
    if audio.shape[1] <= frame_length // 2:
        raise RuntimeError(f"audio: {audio.shape[1]} samples, the reflect padding needs more than frame_length / 2 = "
                           f"{frame_length // 2}")
    return audio.contiguous()


def pyin_cmnd(audio: torch.Tensor, sample_rate: float = 16000, minimum_frequency: float = 65.0,
              maximum_frequency: float = 2093.0, frame_length: int = 1024, hop_length: int = 128) -> torch.Tensor:
    """(B, N) -> yin (B, T, lags) fp32, lags = max_period - min_period + 1, T = 1 + N // hop_length"""
    cfg = _config(sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length)
    return binding().pyin_cmnd(_audio(audio, cfg[3]), *cfg)


def pyin_observe(yin: torch.Tensor, sample_rate: float = 16000, minimum_frequency: float = 65.0,
                 maximum_frequency: float = 2093.0, frame_length: int = 1024, hop_length: int = 128):
    """yin -> (cand_bin (B, T, lags) int32, cand_prob (B, T, lags) fp64, count (B, T) int32, voiced_prob (B, T) fp64)"""
    if not yin.is_cuda or yin.dtype != torch.float32 or yin.dim() != 3:
        raise RuntimeError("yin: expected a (B, T, lags) float32 CUDA tensor (no CPU fallback)")
    cfg = _config(sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length)
    return binding().pyin_observe(yin.contiguous(), _table(cfg, yin.device), *cfg)


def pyin_viterbi(cand_bin, cand_prob, count, voiced_prob, sample_rate: float = 16000, minimum_frequency: float = 65.0,
                 maximum_frequency: float = 2093.0, frame_length: int = 1024, hop_length: int = 128,
                 fill_na: Optional[float] = None):
    """sparse observations -> (states (B, T) int32: voiced bins then unvoiced bins, f0 (B, T) fp32)"""
    for name, t, dt in (("cand_bin", cand_bin, torch.int32), ("cand_prob", cand_prob, torch.float64),
                        ("count", count, torch.int32), ("voiced_prob", voiced_prob, torch.float64)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise RuntimeError(f"{name}: expected a contiguous {dt} CUDA tensor (no CPU fallback)")
    cfg = _config(sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length)
    return binding().pyin_viterbi(cand_bin, cand_prob, count, voiced_prob, _table(cfg, cand_bin.device), *cfg,
                                  fill_na is not None, float(fill_na) if fill_na is not None else 0.0)


def pyin_frames(audio: torch.Tensor, sample_rate: float = 16000, minimum_frequency: float = 65.0,
                maximum_frequency: float = 2093.0, frame_length: int = 1024, hop_length: int = 128,
                fill_na: Optional[float] = None):
    """(B, N) fp32 CUDA tensor -> (f0 (B, T) fp32, voiced_prob (B, T) fp64, states (B, T) int32), T = 1 + N // hop_length;
    a frame is voiced when its state is below n_pitch_bins"""
    cfg = _config(sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length)
    audio = _audio(audio, cfg[3])
    return binding().pyin(audio, _table(cfg, audio.device), *cfg, fill_na is not None,
                          float(fill_na) if fill_na is not None else 0.0)


@gin.configurable
def extract_f0_with_crepe(audio: np.ndarray, sample_rate: float, hop_length: int = 128, minimum_frequency: float = 50.0,
                          maximum_frequency: float = 2000.0, full_model: bool = True, batch_size: int = 2048,
                          device: Union[str, torch.device] = "cpu",
                          interpolate_fn: Optional[Callable] = linear_interpolation):
    """f0_extraction.py:16-57.  Not available: CREPE is a trained network (torchcrepe and its weights)."""
    raise RuntimeError("extract_f0_with_crepe is not available: CREPE needs torchcrepe and its weights, which this package "
                       "does not ship; use extract_f0_with_pyin")


@gin.configurable
def extract_f0_with_pyin(audio, sample_rate: float, minimum_frequency: float = 65.0, maximum_frequency: float = 2093.0,
                         frame_length: int = 1024, hop_length: int = 128, fill_na: Optional[float] = None,
                         interpolate_fn: Optional[Callable] = linear_interpolation):
    """f0_extraction.py:60-92: -> (f0, voiced_prob).  fill_na=None keeps the decoded pitch on unvoiced frames, a number
    replaces it there.  interpolate_fn, if given, is called exactly like the reference calls it, on the host."""
    is_numpy = isinstance(audio, np.ndarray)
    x = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).cuda() if is_numpy else audio
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    f0, voiced_prob, _ = pyin_frames(x, sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length, fill_na)
    if interpolate_fn:
        out = []
        for rows in (f0.cpu().numpy().astype(np.float64), voiced_prob.cpu().numpy()):
            res = np.stack([interpolate_fn(r, frame_length, hop_length, original_length=x.shape[1]) for r in rows])
            res = res[0] if squeeze else res
            out.append(res if is_numpy else torch.as_tensor(res))
        return out[0], out[1]
    if squeeze:
        f0, voiced_prob = f0[0], voiced_prob[0]
    if is_numpy:
        return f0.cpu().numpy().astype(np.float64), voiced_prob.cpu().numpy()
    return f0, voiced_prob
