"""From a wav file to the segments of a dataset on the MI355X (mirror of
neural_waveshaping_synthesis/data/utils/preprocess_audio.py): integer audio to float32, stereo to mono, level
normalisation, `resample_audio`, where the reference calls `resampy.resample` and `csrc/resample.hip` runs here
(DESIGN.md 3.10 is the definition; parity with resampy is unpinned), then the chain that strings the extractors together
(:69-237): F0, loudness and MFCC of the whole file, cut into segments, segments kept by their mean F0 confidence.

`resample_audio` accepts a 1-D numpy array like the reference (returns numpy float32), or a (N,) / (B, N) float32 CUDA
tensor (returns a tensor).  No CPU fallback.  `preprocess_audio` is the generator `create_dataset` consumes.

Departures from the reference: the default F0 extractor is pYIN (CREPE is not available here); a signal
shorter than one segment gives no segment instead of an exception; the audio and the control features of a file are trimmed
to the same number of segments; `preprocess_audio` passes its confidence threshold on.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch
from scipy.io import wavfile

from ... import ginlite as gin
from ...engine import binding
from .f0_extraction import extract_f0_with_pyin
from .loudness_extraction import extract_perceptual_loudness
from .mfcc_extraction import extract_mfcc

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


def segment_signal(signal: np.ndarray, sample_rate: float, segment_length_in_seconds: float, hop_length_in_seconds: float):
    """:69-80.  (..., L) -> (..., segment, n): column j holds signal[..., j hop : j hop + segment], with segment and hop
    int(sample_rate x seconds) samples and n = 1 + (L - segment) // hop - the array librosa.util.frame returns.  A signal
    shorter than one segment gives n = 0 (librosa raises)."""
    signal = np.asarray(signal)
    segment, hop = int(sample_rate * segment_length_in_seconds), int(sample_rate * hop_length_in_seconds)
    if segment < 1 or hop < 1:
        raise ValueError(f"segments of {segment} samples every {hop} samples: both must be at least 1")
    length = signal.shape[-1]
    n = 1 + (length - segment) // hop if length >= segment else 0
    index = np.arange(segment)[:, None] + hop * np.arange(n)[None, :]
    return signal[..., index]


def filter_segments(threshold: float, key_segments: np.ndarray, segments: Sequence[np.ndarray]):
    """:83-93.  Keeps, in every array of `segments`, the entries of the last axis at which the mean of `key_segments`
    (segment, n) over a segment is above `threshold`"""
    mask = key_segments.mean(axis=0) > threshold
    return [x[..., mask] for x in segments]


def _read_mono(file: str):
    rate, audio = wavfile.read(file)
    return rate, make_monophonic(convert_to_float32_audio(audio))


def preprocess_single_audio_file(file: str, control_decimation_factor: float, target_sr: float = 16000.0,
                                 segment_length_in_seconds: float = 4.0, hop_length_in_seconds: float = 2.0,
                                 confidence_threshold: float = 0.85, f0_extractor: Callable = extract_f0_with_pyin,
                                 loudness_extractor: Callable = extract_perceptual_loudness,
                                 mfcc_extractor: Callable = extract_mfcc, normalisation_factor: Optional[float] = None):
    """:96-199.  One wav file -> five lists with one entry per kept segment: audio (L,), f0 (Lc,), confidence (Lc,),
    loudness (Lc,), mfcc (n_mfcc, Lc).  The extractors are called with the audio alone; everything else they need is bound
    through gin.  Control features are segmented at target_sr / control_decimation_factor."""
    print(f"{file}: reading")
    original_sr, audio = _read_mono(file)
    if normalisation_factor:
        audio = normalise_signal(audio, normalisation_factor)
    audio = resample_audio(np.ascontiguousarray(audio, dtype=np.float32), original_sr, target_sr)
    print(f"{file}: {audio.size} samples at {target_sr:g} Hz; F0 ({f0_extractor.__name__}), loudness "
          f"({loudness_extractor.__name__}), MFCC ({mfcc_extractor.__name__})")
    f0, confidence = f0_extractor(audio)
    loudness = loudness_extractor(audio)
    mfcc = mfcc_extractor(audio)
    control_sr = target_sr / (control_decimation_factor or 1)
    cut = [segment_signal(audio, target_sr, segment_length_in_seconds, hop_length_in_seconds)]
    cut += [segment_signal(x, control_sr, segment_length_in_seconds, hop_length_in_seconds) for x in (f0, confidence, loudness, mfcc)]
    # N samples give q = N // hop whole control hops but q + 1 control frames: when q = Lc - 1 (mod Hc) the control features
    # have one segment more than the audio.  Every array keeps the segments all of them have.
    n = min(x.shape[-1] for x in cut)
    cut = [x[..., :n] for x in cut]
    kept = filter_segments(confidence_threshold, cut[2], cut)
    print(f"{file}: {kept[0].shape[-1]} of {n} segments above the confidence threshold {confidence_threshold}")
    return tuple([x[..., j] for j in range(x.shape[-1])] for x in kept)


@gin.configurable
def preprocess_audio(files: list, control_decimation_factor: float, target_sr: float = 16000,
                     segment_length_in_seconds: float = 4.0, hop_length_in_seconds: float = 2.0,
                     confidence_threshold: float = 0.85, f0_extractor: Callable = extract_f0_with_pyin,
                     loudness_extractor: Callable = extract_perceptual_loudness, normalise_audio: bool = False):
    """:202-237.  A generator over `files`: the five lists of preprocess_single_audio_file for each.  normalise_audio
    divides every file by the largest absolute sample of all of them."""
    factor = None
    if normalise_audio:
        factor = max(float(np.abs(_read_mono(file)[1]).max()) for file in files) if files else None
    for file in files:
        yield preprocess_single_audio_file(
            file, control_decimation_factor=control_decimation_factor, target_sr=target_sr,
            segment_length_in_seconds=segment_length_in_seconds, hop_length_in_seconds=hop_length_in_seconds,
            confidence_threshold=confidence_threshold, f0_extractor=f0_extractor, loudness_extractor=loudness_extractor,
            normalisation_factor=factor)
