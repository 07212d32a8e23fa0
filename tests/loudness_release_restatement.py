"""Restatement of the releasing loudness reference of DESIGN.md 3.26 on top of tests/loudness_stream_restatement.py: the level
recurrence, the window maximum that is a frame's reference and the dB pass, once as a closed form over a whole clip
(`stream`, `stream_of_power`) and once push by push as the chunks arrive (`Stream`, `run_chunks`).  The recurrence runs in
`dtype`: float64 for the restatement the kernels are held near, np.float32 for the one their references are held equal to."""
import numpy as np

import loudness_stream_restatement as ls
from oracle import loudness_oracle as lo

TINY = 2.0 ** -126          # below this a decayed level is flushed to 0, whatever the denormal mode


def release_factor(release_db_per_s, hop, sample_rate):
    """rho: computed in float64, rounded once to float32"""
    return float(np.float32(10.0 ** (-float(release_db_per_s) * hop / (10.0 * float(sample_rate)))))


def decay(m, rho, dtype=np.float64):
    """g(m) = flush(fl(rho m)): one product in `dtype`, flushed below 2^-126"""
    d = dtype(rho) * dtype(m)
    return dtype(0.0) if d < TINY else d


def step(M, p, floor, rho, dtype=np.float64):
    """M(t) from M(t - 1) and p(t).  At rho = 1 the product is exact and nothing is flushed: 3.25's max(M(t - 1), p(t))"""
    if not rho < 1.0:
        return max(dtype(M), dtype(p))
    return max(dtype(p), dtype(floor), decay(M, rho, dtype))


def levels(p, rho=1.0, floor=0.0, track=True, dtype=np.float64):
    """M(t) of the frames' peak powers p(t), M(-1) = floor; without track the constant `floor` (3.25's fixed reference)"""
    out, M = np.empty(len(p), dtype=dtype), dtype(floor)
    for t in range(len(p)):
        if track:
            M = step(M, p[t], floor, rho, dtype)
        out[t] = M
    return out


def levels_closed_form(p, rho, floor=0.0, dtype=np.float32):
    """consequence 6: M(t) = max(F, max_{k <= t} g^(t - k)(max(p(k), F))) - every frame contributes its own decaying term"""
    out = np.empty(len(p), dtype=dtype)
    terms = []                                        # g^(t - k)(max(p(k), F)) for k = 0 .. t
    for t in range(len(p)):
        terms = [decay(v, rho, dtype) for v in terms] + [max(dtype(p[t]), dtype(floor))]
        out[t] = max([dtype(floor)] + terms)
    return out


def window_refs(M, N, n_fft, hop, L):
    """ref(e): the largest level over e .. e + L while frame e + L is one of the F(N) frames computed before the stream ended,
    over e .. T - 1 for the frames the flush releases"""
    F, T = ls.frames_computed(N, n_fft, hop), len(M)
    return np.array([M[e:e + L + 1].max() if e + L <= F - 1 else M[e:].max() for e in range(T)], dtype=M.dtype)


def stream_of_power(P, N, n_fft, hop, L, rho=1.0, floor=0.0, track=True, amin=1e-5, normalise=True):
    """a clip of N samples whose power spectrogram P (bins, T) is at hand -> (loudness (T,), ref (T,)), in float64"""
    ref = window_refs(levels(P.max(axis=0), rho, floor, track), N, n_fft, hop, L)
    return ls.decibels(P, ref, amin, 80.0, normalise), ref


def stream(audio, n_fft, hop, L, rho=1.0, floor=0.0, track=True, amin=1e-5, normalise=True):
    audio = np.asarray(audio, dtype=np.float64)
    return stream_of_power(lo.stft_magnitude(audio, n_fft, hop) ** 2, audio.size, n_fft, hop, L, rho, floor, track, amin, normalise)


class Stream(ls.Stream):
    """the definition followed as the samples arrive: ls.Stream with the level recurrence and the window maximum"""

    def __init__(self, n_fft, hop, L, rho=1.0, floor=0.0, track=True, amin=1e-5, normalise=True):
        super().__init__(n_fft, hop, L, track=track, initial=floor, amin=amin, normalise=normalise)
        self.rho, self.floor = rho, float(floor)

    def _grow(self, frames, end=None):
        for t in range(len(self.P), frames):
            self.P.append(self._frame(t, end))
            if self.track:
                self.level = float(step(self.level, float(self.P[-1].max()), self.floor, self.rho))
            self.M.append(self.level)

    def _release(self, upto, flush):
        es = range(self.emitted, upto)
        ref = np.array([max(self.M[e:] if flush else self.M[e:e + self.L + 1]) for e in es])
        P = np.stack([self.P[e] for e in es], axis=1) if len(es) else np.zeros((self.n_fft // 2 + 1, 0))
        self.emitted = upto
        return ls.decibels(P, ref, self.amin, 80.0, self.normalise), ref


def run_chunks(audio, chunks, n_fft, hop, L, **kw):
    """`chunks` of a clip through a Stream + the flush -> (loudness, ref, frames released per push)"""
    s, at, outs = Stream(n_fft, hop, L, **kw), 0, []
    for n in chunks:
        outs.append(s.push(audio[at:at + n]))
        at += n
    assert at == len(audio)
    outs.append(s.flush())
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), [len(o[0]) for o in outs]


def recovery_input(n_fft, hop, N):
    """the recovery inputs of 3.26: (x with a click of four samples at 1.0 from sample 10 hop, x' = the noise alone)"""
    clean = np.random.default_rng(5).uniform(-0.02, 0.02, N)
    x = clean.copy()
    x[10 * hop:10 * hop + 4] = 1.0
    return x, clean
