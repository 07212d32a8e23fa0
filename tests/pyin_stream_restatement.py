"""Restatement of the fixed-lag pYIN stream of DESIGN.md 3.24, on top of tests/pyin_restatement.py: the offline forward pass
(value vectors and backpointers, float64), read out by a lagged backtrace, and the stream's arithmetic - frames computed,
frames emitted, state size - by brute force over sample counts rather than by the closed forms the library uses."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import pyin_restatement as pr

RING = 512               # frames of backpointers a row keeps
STEP_FRAMES = 256        # most new frames of one pass: a step takes at most STEP_FRAMES hop samples
MAX_LAG = 255


def forward(cand_bin, cand_prob, count, voiced_prob, c):
    """the forward pass of pr.viterbi -> (arg (T,): argmax V_t, lowest index on ties; back (T, 2 n_bins): best source of every
    state of frame t >= 1)"""
    lv, lu = pr.log_observations(cand_bin, cand_prob, count, voiced_prob, c)
    T, nb, h, width = len(count), c.n_bins, c.h, c.width
    w, rowsum = pr._window(c), pr._rowsum(c)
    src = np.arange(nb)[:, None] + np.arange(width)[None, :] - h
    ok = (src >= 0) & (src < nb)
    pw = np.where(ok, w[np.abs(np.arange(width) - h)][None, :] / rowsum[np.clip(src, 0, nb - 1)], 0.0)
    with np.errstate(divide="ignore"):
        lt_same = np.where(ok, np.log(pw * (1 - pr.SWITCH_PROB) + pr.TINY64), -np.inf)
        lt_cross = np.where(ok, np.log(pw * pr.SWITCH_PROB + pr.TINY64), -np.inf)
    ltiny = np.log(pr.TINY64)
    V = pr._log_init(c) + np.concatenate([lv[0], np.full(nb, lu[0])])
    back = np.zeros((T, 2 * nb), dtype=np.int64)
    arg = np.zeros(T, dtype=np.int64)
    arg[0] = int(np.argmax(V))
    pad = np.full(h, -np.inf)
    for t in range(1, T):
        wv = sliding_window_view(np.concatenate([pad, V[:nb], pad]), width)
        wu = sliding_window_view(np.concatenate([pad, V[nb:], pad]), width)
        g = int(np.argmax(V))
        jump = V[g] + ltiny
        new = np.empty(2 * nb)
        for half, (la, lb) in enumerate(((lt_same, lt_cross), (lt_cross, lt_same))):
            cand = np.concatenate([wv + la, wu + lb], axis=1)
            k = np.argmax(cand, axis=1)
            best = cand[np.arange(nb), k]
            source = np.where(k < width, 0, nb) + np.arange(nb) + (k % width) - h
            use_jump = jump > best
            back[t, half * nb:(half + 1) * nb] = np.where(use_jump, g, source)
            new[half * nb:(half + 1) * nb] = np.where(use_jump, jump, best)
        V = new + np.concatenate([lv[t], np.full(nb, lu[t])])
        arg[t] = int(np.argmax(V))
    return arg, back


def state_at(arg, back, start, e):
    """the state at frame e of the backtrace that starts at argmax V_start"""
    s = int(arg[start])
    for t in range(start, e, -1):
        s = int(back[t, s])
    return s


def lagged(arg, back, L, computed=None):
    """the stream's states of a whole clip: frame e from argmax V_{e + L} while e + L is one of the `computed` frames that
    existed before the stream ended (default: all of them), every later frame from argmax V_{T - 1}"""
    T = len(arg)
    computed = T if computed is None else computed
    return np.array([state_at(arg, back, e + L if e + L <= computed - 1 else T - 1, e) for e in range(T)], dtype=np.int64)


# ---- the stream's arithmetic, by brute force ----------------------------------------------------------------------------
def frames_computed(n, c):
    """F(n): frames all of whose samples exist.  Frame t covers [hop t - W, hop t + W); the reflection at the left edge of
    frame 0 reads sample W as well"""
    f = 0
    while (n > c.W) if f == 0 else (c.hop * f + c.W <= n):
        f += 1
    return f


def frames_total(n, c):
    """T of a stream that ended after n samples"""
    return len(range(0, n + 1, c.hop))


def frames_emitted(n, c, L, final=False):
    if final:
        return frames_total(n, c)
    return sum(1 for e in range(frames_computed(n, c)) if e + L <= frames_computed(n, c) - 1)


def max_chunk(c):
    return STEP_FRAMES * c.hop


def state_bytes(B, c):
    pad8 = lambda k: (k + 7) // 8 * 8
    row = (4 * 8                         # n_seen, frames computed, frames emitted, finished
           + 2 * 8                       # max V and argmax V of the last frame
           + 2 * c.n_bins * 8            # V - log rowsum
           + RING * 8 + RING * 4         # voiced_prob ring, jump-word ring
           + pad8(4 * c.frame_length)    # sample history
           + pad8(RING * 2 * c.n_bins))  # backpointer ring
    return B * row


def max_new_frames(n, c, final=False):
    """most frames one pass of a step of n samples computes, over every count of samples the stream may have seen before it (a
    final step is two passes: its samples, then the flush)"""
    top = 2 * c.frame_length + 2 * c.hop
    F = [frames_computed(k, c) for k in range(top + n + 1)]
    most = max(F[k + n] - F[k] for k in range(top + 1))
    if final:
        most = max([most] + [frames_total(k + n, c) - F[k + n] for k in range(top + 1) if k + n > c.W])
    return most


def workspace_bytes(B, frames, c):
    """scratch of a pass of `frames` new frames: candidate probabilities, voiced_prob, yin, candidate bins, counts, each padded to 256"""
    pad = lambda k: (k + 255) // 256 * 256
    n = B * frames * c.lags
    return pad(8 * n) + pad(8 * B * frames) + pad(4 * n) + pad(4 * n) + pad(4 * B * frames)
