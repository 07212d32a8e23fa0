"""Float64 numpy / scipy restatement of the resampler's definition of DESIGN.md 3.10: resampy 0.2.2's `kaiser_best`
interpolation as published, with two stated departures (n_out = (N L) // M exactly; the position of output t is the exact
rational t M / L instead of an accumulated float).  Parity with resampy itself is unpinned: it is not installed where this
project is built.  `resample(..., sum_dtype=np.float32)` is the same loop with fp64 weights and an fp32 running sum, which is
resampy's own arithmetic on float32 audio: the yardstick of the GPU test's error bound.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
from scipy.signal.windows import kaiser

NUM_ZEROS = 64
NB = 2 ** 9
NWIN = NUM_ZEROS * NB + 1
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492


@functools.lru_cache(maxsize=None)
def _unit_window():
    k = np.arange(NWIN, dtype=np.float64)
    return ROLLOFF * np.sinc(ROLLOFF * (NUM_ZEROS * k / (NWIN - 1))) * kaiser(2 * (NWIN - 1) + 1, BETA)[NWIN - 1:]


@functools.lru_cache(maxsize=None)
def config(sr_in, sr_out):
    """rates -> L, M, ratio, scale, step, the half window and its differences, the per-phase wing offsets and lengths,
    left / right / taps"""
    sr_in, sr_out = int(sr_in), int(sr_out)
    assert sr_in >= 1 and sr_out >= 1
    g = math.gcd(sr_in, sr_out)
    c = SimpleNamespace(sr_in=sr_in, sr_out=sr_out, L=sr_out // g, M=sr_in // g)
    c.ratio = float(sr_out) / sr_in
    c.scale = min(1.0, c.ratio)
    c.win = _unit_window().copy()
    if c.ratio < 1:
        c.win *= c.ratio
    c.delta = np.zeros_like(c.win)
    c.delta[:-1] = np.diff(c.win)
    c.step = int(c.scale * NB)
    phi = np.arange(c.L, dtype=np.float64) / c.L
    frac = c.scale * phi
    idx = frac * NB
    c.off_l = idx.astype(np.int64)
    c.eta_l = idx - c.off_l
    idx = (c.scale - frac) * NB
    c.off_r = idx.astype(np.int64)
    c.eta_r = idx - c.off_r
    c.n_l = (NWIN - c.off_l) // c.step
    c.n_r = (NWIN - c.off_r) // c.step
    c.left, c.right = int(c.n_l.max()), int(c.n_r.max())
    c.taps = c.left + c.right
    return c


def dims(sr_in, sr_out):
    c = config(sr_in, sr_out)
    return c.L, c.M, c.taps, c.left, c.right, c.step


def length(n, sr_in, sr_out):
    c = config(sr_in, sr_out)
    return (int(n) * c.L) // c.M


def bank(sr_in, sr_out):
    """(L, taps) float64: row r = the weights of phase numerator r, column c on x[n + c - (left - 1)], unused columns 0"""
    c = config(sr_in, sr_out)
    b = np.zeros((c.L, c.taps), dtype=np.float64)
    for r in range(c.L):
        i = c.off_l[r] + np.arange(c.n_l[r]) * c.step
        b[r, c.left - 1 - np.arange(c.n_l[r])] = c.win[i] + c.eta_l[r] * c.delta[i]
        i = c.off_r[r] + np.arange(c.n_r[r]) * c.step
        b[r, c.left + np.arange(c.n_r[r])] = c.win[i] + c.eta_r[r] * c.delta[i]
    return b


def resample(x, sr_in, sr_out, sum_dtype=np.float64):
    """x (..., N) -> (..., (N L) // M).  The taps of an output are added in resampy's order (left wing outwards from x[n],
    then right wing outwards from x[n + 1]); every product is float64, the running sum is rounded to `sum_dtype` after
    every addition.  All outputs advance together, one tap per step."""
    c = config(sr_in, sr_out)
    x = np.asarray(x)
    N = x.shape[-1]
    n_out = (N * c.L) // c.M
    t = np.arange(n_out, dtype=np.int64)
    n, r = np.divmod(t * c.M, c.L)
    xp = np.concatenate([x.astype(np.float64), np.zeros(x.shape[:-1] + (1,))], axis=-1)      # index N: the zero outside
    y = np.zeros(x.shape[:-1] + (n_out,), dtype=sum_dtype)
    for off, eta, count, sign, first in ((c.off_l[r], c.eta_l[r], c.n_l[r], -1, n), (c.off_r[r], c.eta_r[r], c.n_r[r], 1, n + 1)):
        for i in range(int(count.max(initial=0))):
            live = i < count
            k = np.where(live, off + i * c.step, 0)
            w = np.where(live, c.win[k] + eta * c.delta[k], 0.0)
            src = first + sign * i
            src = np.where(live & (src >= 0) & (src < N), src, N)
            y = (y.astype(np.float64) + w * xp[..., src]).astype(sum_dtype)
    return y
