"""Restatement of the loudness stream of DESIGN.md 3.25 in float64, on top of oracle/loudness_oracle.py's STFT: the causal
reference level and the dB pass as a closed form over a whole clip (`stream`), the same definition followed sample by sample
as the chunks arrive (`Stream`, which computes every frame from the samples that exist at that moment), and the stream's
arithmetic - frames computed, frames emitted, state and scratch sizes - by brute force over sample counts rather than by the
closed forms the library uses."""
import numpy as np

from oracle import loudness_oracle as lo

RING = 512               # frames of P and M a row keeps
STEP_FRAMES = 256        # a step takes at most STEP_FRAMES hop samples; a flush computes at most that many frames
MAX_LAG = 255


# ---- the stream's arithmetic, by brute force ----------------------------------------------------------------------------
def frames_computed(n, n_fft, hop):
    """F(n): frames all of whose samples exist.  Frame t covers [hop t - W, hop t + W); the reflection at the left edge of
    frame 0 reads sample W as well"""
    W, f = n_fft // 2, 0
    while (n > W) if f == 0 else (hop * f + W <= n):
        f += 1
    return f


def frames_total(n, hop):
    """T of a stream that ended after n samples"""
    return len(range(0, n + 1, hop))


def frames_emitted(n, n_fft, hop, L, final=False):
    if final:
        return frames_total(n, hop)
    F = frames_computed(n, n_fft, hop)
    return sum(1 for e in range(F) if e + L <= F - 1)


def max_chunk(hop):
    return STEP_FRAMES * hop


def state_layout(n_fft):
    """byte offsets of a row's parts, each padded to 8 bytes: counters | M, track | history | M ring | P ring | end"""
    pad8 = lambda k: (k + 7) // 8 * 8
    off, at = {}, 0
    for name, size in (("counters", 4 * 8), ("reference", 4 + 4), ("history", 4 * n_fft), ("m_ring", 4 * RING),
                       ("p_ring", 4 * RING * (n_fft // 2 + 1))):
        off[name] = at
        at += pad8(size)
    off["row"] = at
    return off


def state_bytes(B, n_fft):
    return B * state_layout(n_fft)["row"]


def max_new_frames(n, n_fft, hop, final=False):
    """most frames one pass of a step of n samples computes, over every count of samples the stream may have seen before it (a
    final step is two passes: its samples, then the flush)"""
    top = 2 * n_fft + 2 * hop
    F = [frames_computed(k, n_fft, hop) for k in range(top + n + 1)]
    most = max(F[k + n] - F[k] for k in range(top + 1))
    if final:
        most = max([most] + [frames_total(k + n, hop) - F[k + n] for k in range(top + 1) if k + n > n_fft // 2])
    return most


def workspace_bytes(B, frames):
    """scratch of a pass of `frames` new frames: one word per row and frame for p(t), padded to 256"""
    return (4 * B * frames + 255) // 256 * 256


# ---- the definition ------------------------------------------------------------------------------------------------------
def decibels(P, ref, amin=1e-5, top_db=80.0, normalise=True):
    """P (bins, frames) powers, ref (frames,) reference powers -> loudness (frames,)"""
    db = 10.0 * np.log10(np.maximum(amin * amin, P)) - 10.0 * np.log10(np.maximum(amin * amin, np.asarray(ref, dtype=np.float64)))[None, :]
    l = np.cumsum(np.maximum(db, -top_db), axis=0)[-1] / P.shape[0]      # the sum over the bins in order, as the definition has it

    return (l + 80.0) / 80.0 if normalise else l


def levels(p, track=True, initial=0.0):
    """M(t) of the frames' peak powers p(t)"""
    return np.maximum(np.maximum.accumulate(p), initial) if track else np.full(len(p), float(initial))


def stream(audio, n_fft, hop, L, track=True, initial=0.0, amin=1e-5, normalise=True):
    """a whole clip through the stream -> (loudness (T,), ref (T,)): frame e against M(e + L) while frame e + L is one of the
    F(N) frames computed before the stream ended, against M(T - 1) after"""
    audio = np.asarray(audio, dtype=np.float64)
    return stream_of_power(lo.stft_magnitude(audio, n_fft, hop) ** 2, audio.size, n_fft, hop, L, track, initial, amin, normalise)


def stream_of_power(P, N, n_fft, hop, L, track=True, initial=0.0, amin=1e-5, normalise=True):
    """`stream` of a clip of N samples whose power spectrogram P (bins, T) is at hand"""
    T = P.shape[1]
    M = levels(P.max(axis=0), track, initial)
    F = frames_computed(N, n_fft, hop)
    ref = np.array([M[e + L] if e + L <= F - 1 else M[T - 1] for e in range(T)])
    return decibels(P, ref, amin, 80.0, normalise), ref


class Stream:
    """the definition followed as the samples arrive: push(chunk) / flush() -> (loudness, ref) of the frames released"""

    def __init__(self, n_fft, hop, L, track=True, initial=0.0, amin=1e-5, normalise=True):
        self.n_fft, self.hop, self.L, self.track, self.amin, self.normalise = n_fft, hop, L, track, amin, normalise
        self.x = np.zeros(0)
        self.P, self.M, self.level, self.emitted = [], [], float(initial), 0
        self.window = lo.hann_periodic(n_fft)

    def _frame(self, t, end=None):
        """power of frame t from the samples that exist; `end`: the stream's length, whose right edge is reflected"""
        W = self.n_fft // 2
        i = np.abs(self.hop * t - W + np.arange(self.n_fft))
        if end is not None:
            i = np.where(i >= end, 2 * (end - 1) - i, i)
        assert i.min() >= 0 and i.max() < self.x.size
        return np.abs(np.fft.rfft(self.window * self.x[i])) ** 2

    def _grow(self, frames, end=None):
        for t in range(len(self.P), frames):
            self.P.append(self._frame(t, end))
            if self.track:
                self.level = max(self.level, float(self.P[-1].max()))
            self.M.append(self.level)

    def _release(self, upto, flush):
        es = range(self.emitted, upto)
        ref = np.array([self.M[-1] if flush else self.M[e + self.L] for e in es])
        P = np.stack([self.P[e] for e in es], axis=1) if len(es) else np.zeros((self.n_fft // 2 + 1, 0))
        self.emitted = upto
        return decibels(P, ref, self.amin, 80.0, self.normalise), ref

    def push(self, chunk):
        self.x = np.concatenate([self.x, np.asarray(chunk, dtype=np.float64)])
        self._grow(frames_computed(self.x.size, self.n_fft, self.hop))
        return self._release(max(self.emitted, len(self.P) - self.L), False)

    def flush(self):
        assert self.x.size > self.n_fft // 2
        self._grow(frames_total(self.x.size, self.hop), end=self.x.size)
        return self._release(len(self.P), True)


def run_chunks(audio, chunks, n_fft, hop, L, **kw):
    """`chunks` of a clip through a Stream + the flush -> (loudness, ref, frames released per push)"""
    s, at, outs = Stream(n_fft, hop, L, **kw), 0, []
    for n in chunks:
        outs.append(s.push(audio[at:at + n]))
        at += n
    assert at == len(audio)
    outs.append(s.flush())
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), [len(o[0]) for o in outs]
