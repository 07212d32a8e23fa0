"""MFCC feature on the MI355X (mirror of neural_waveshaping_synthesis/data/utils/mfcc_extraction.py).

`extract_mfcc` keeps the reference's signature and gin binding names (:7-13; no defaults, as there).  Where the reference
calls `librosa.feature.mfcc`, `csrc/mfcc.hip` runs: the loudness feature's power STFT, a sparse Slaney mel pass, the dB
clip against the utterance's maximum and an orthonormal DCT-II (DESIGN.md 3.11 is the definition; parity with librosa is
unpinned).  Accepts a 1-D numpy array like the reference (returns a numpy (n_mfcc, T) float32 array), or a (N,) / (B, N)
float32 CUDA tensor (returns a tensor (n_mfcc, T) / (B, n_mfcc, T)).  No CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import ginlite as gin
from ...engine import binding
from .loudness_extraction import _dft_operand

N_MELS = 128          # librosa.feature.melspectrogram's default, which the reference never overrides

_TABLE_CACHE: dict = {}


def _table(cfg, device) -> torch.Tensor:
    """filter spans, weights and DCT rows of a configuration on `device` (built once on the host)"""
    key = (cfg, str(device))
    t = _TABLE_CACHE.get(key)
    if t is None:
        t = binding().mfcc_table(*cfg).to(device)
        torch.cuda.current_stream(device).synchronize()     # shared by every later caller, whatever its stream
        _TABLE_CACHE[key] = t
    return t


def mfcc_frames(audio: torch.Tensor, sample_rate: float, n_fft: int, hop_length: int, n_mfcc: int,
                n_mels: int = N_MELS) -> torch.Tensor:
    """(B, N) fp32 CUDA tensor -> (B, n_mfcc, 1 + N // hop_length)"""
    if not isinstance(audio, torch.Tensor) or not audio.is_cuda or audio.dtype != torch.float32 or audio.dim() != 2:
        raise RuntimeError("audio: expected a (B, N) float32 CUDA tensor (no CPU fallback)")
    cfg = (float(sample_rate), int(n_fft), int(n_mfcc), int(n_mels))
    audio = audio.contiguous()
    table = _table(cfg, audio.device)          # refuses an unsupported configuration before the DFT operand is asked for
    return binding().mfcc(audio, _dft_operand(cfg[1], audio.device), table, cfg[0], cfg[1], int(hop_length), cfg[2], cfg[3])


@gin.configurable
def extract_mfcc(audio, sample_rate: float, n_fft: int, hop_length: int, n_mfcc: int):
    """mfcc_extraction.py:7-13"""
    is_numpy = isinstance(audio, np.ndarray)
    if is_numpy:
        if audio.ndim != 1:
            raise ValueError(f"audio: expected a 1-D array, got {audio.shape}")
        if not torch.cuda.is_available():
            raise RuntimeError("extract_mfcc runs on the GPU: no device is available and there is no CPU fallback")
        x = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32)).cuda()
    else:
        x = audio
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (1, 2):
        raise RuntimeError("audio: expected a 1-D numpy array or a (N,) / (B, N) float32 CUDA tensor (no CPU fallback)")
    squeeze = x.dim() == 1
    if squeeze:
        x = x.unsqueeze(0)
    out = mfcc_frames(x, sample_rate, n_fft, hop_length, n_mfcc)
    if squeeze:
        out = out[0]
    return out.cpu().numpy() if is_numpy else out
