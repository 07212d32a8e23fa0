"""Shared by the long-stream tests (plain numpy / torch-CPU, no GPU): the 560-frame inputs, the float64 reverb the stream's
output is held to, and models of the defects those checks are there to catch.

A stream keeps a ring of 65 536 reverb-input samples per row and sums the reverb over the last 31 999 of them in 125 parts of
256 taps.  560 frames = 71 680 samples: longer than the impulse response (frame 250) and past the ring's wrap (frame 512)."""
import numpy as np
import torch
from scipy.signal import fftconvolve

from conftest import rms

F_LONG = 560
RING = 65536                      # NWS_STREAM_RING of csrc/nws_common.h
SEGMENTS = ((0, 60), (60, 250), (250, 512), (512, 560))     # frames: what was measured before | up to the IR's length | up to the wrap | after it
SCHEDULES = {"2x280": [2] * 280, "16x35": [16] * 35, "249_249_62": [249, 249, 62], "mixed": [1, 7, 16, 4, 31, 1] * 9 + [20]}
assert all(sum(c) == F_LONG for c in SCHEDULES.values())


def long_inputs(B, F=F_LONG, seed=560):
    """f0 / control / the two hidden draws, built the way test_stream_equals_one_shot builds them"""
    g = torch.Generator().manual_seed(seed)
    f0 = (120 + 600 * torch.rand(B, 1, 1, generator=g)) * (1 + 0.03 * torch.randn(B, 1, F, generator=g))
    control = torch.randn(B, 2, F, generator=g)
    pu, nz = torch.rand(101, generator=g), torch.rand(128 * F - 1, generator=g)
    return f0, control, pu, nz


def conv64(pre, ir):
    """float64 linear convolution of every row with [0, ir]: (B, N) -> (B, N + len(ir))"""
    ir_ = np.concatenate([[0.0], np.asarray(ir, np.float64).reshape(-1)])
    return np.stack([fftconvolve(np.asarray(row, np.float64), ir_) for row in pre])


def oracle_reference(oracle, weights, f0, control, pu, nz):
    st = {}
    oracle(f0, control, pu, nz, stages=st)
    pre_ref = st["pre_reverb"].numpy()
    return pre_ref, conv64(pre_ref, weights["reverb.ir"][0])


def reverb_errors(y, pre, tail, ir):
    """RMS errors of a stream's output against ITS OWN dry signal through the float64 reverb: over the whole run, over the
    samples from the ring's wrap on, and of the tail that rings out after the last sample (None: not checked)."""
    N = pre.shape[1]
    full = conv64(pre, ir)
    d = np.asarray(y, np.float64) - (np.asarray(pre, np.float64) + full[:, :N])
    e = {"whole": rms(d), "after_wrap": rms(d[:, RING:])}
    if tail is not None:
        n = min(32000, full.shape[1] - N)
        e["tail"] = rms(np.asarray(tail, np.float64)[:, :n] - full[:, N:N + n])
    return e


def segment_maxabs(a, b):
    """max-abs difference per segment of frames"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return {f"{lo}_{hi}": float(d[:, 128 * lo:128 * hi].max()) for lo, hi in SEGMENTS}


def segment_rel_rms(a, b):
    """rms(a - b) / rms(b) per segment of frames, and over everything"""
    out = {f"{lo}_{hi}": rms(a[:, 128 * lo:128 * hi] - b[:, 128 * lo:128 * hi]) / rms(b[:, 128 * lo:128 * hi]) for lo, hi in SEGMENTS}
    out["all"] = rms(a - b) / rms(b)
    return out


def defective_streams(pre, ir):
    """name -> (y, tail) that a stream with one defect in its reverb state would emit for the dry signal `pre`, in float64:
    what the checks of reverb_errors must NOT let through."""
    pre = np.asarray(pre, np.float64)
    ir = np.asarray(ir, np.float64).reshape(-1)
    N = pre.shape[1]

    def emit(wet):
        return pre + wet[:, :N], wet[:, N:N + 32000]

    out = {}
    short = ir.copy()
    short[256 * ((len(ir) - 1) // 256):] = 0.0                # the last of the 125 parts (taps 31 744 ...) never summed
    out["last_part_dropped"] = emit(conv64(pre, short))
    out["one_sample_late"] = emit(np.pad(conv64(pre, ir), ((0, 0), (1, 0)))[:, :-1])
    lost = pre.copy()
    lost[:, RING:] = 0.0                                      # writes past index 65 535 never land in the ring
    out["input_lost_after_wrap"] = emit(conv64(lost, ir))
    # reads wrap, writes past the wrap do not: a read of sample a >= 65 536 finds sample a - 65 536 still there
    stale = pre.copy()
    stale[:, RING:] = pre[:, :N - RING]
    out["stale_after_wrap"] = emit(conv64(stale, ir))
    return out
