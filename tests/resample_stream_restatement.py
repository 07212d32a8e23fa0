"""Float64 numpy restatement of the streaming resampler's definition of DESIGN.md 3.23, on top of the offline restatement
(tests/resample_restatement.py: `config` gives L, M, taps, left, right, `bank` the L x taps weight rows).

A stream keeps n_seen (input samples consumed), t_next (outputs emitted) and the last taps - 1 input samples.  Output t, with
n, r = divmod(t M, L), is  sum_c bank[r][c] x[n - left + 1 + c]  over everything pushed so far, zero before sample 0.  It leaves
once x[n + right] has been pushed: E(n_seen) outputs in all after n_seen samples.  A final push treats x as zero beyond its end
and emits up to the offline length (n_seen L) // M.
"""
import numpy as np

import resample_restatement as rr


def emitted(n_seen, sr_in, sr_out, final=False):
    """E(n_seen): outputs emitted in all after n_seen input samples; with `final` the offline length.  Python ints."""
    c = rr.config(sr_in, sr_out)
    n_seen = int(n_seen)
    if final:
        return (n_seen * c.L) // c.M
    return 0 if n_seen <= c.right else -((-(n_seen - c.right) * c.L) // c.M)


def max_out(n, sr_in, sr_out, final=False):
    """the most outputs one push of n samples can emit, whatever the stream has seen: E(a + n) - E(a) <= ceil(n L / M) (met at
    a = right), and floor((a + n) L / M) - E(a) <= floor((n + right) L / M) for the final push (met at a = right)"""
    c = rr.config(sr_in, sr_out)
    n = int(n)
    return ((n + c.right) * c.L) // c.M if final else -((-n * c.L) // c.M)


class Stream:
    """One stream of rows of shape `lead` (e.g. (B,)): push(x (..., n), final) -> (..., m) float64."""

    def __init__(self, sr_in, sr_out, lead=()):
        self.c = rr.config(sr_in, sr_out)
        self.bank = rr.bank(sr_in, sr_out)
        self.n_seen = 0
        self.t_next = 0
        self.hist = np.zeros(tuple(lead) + (self.c.taps - 1,))        # x[n_seen - taps + 1 .. n_seen - 1]
        self.finished = False
        self.min_first_word = 0       # smallest staged index any output has read: never negative (taps - 1 samples suffice)

    def push(self, x, final=False):
        assert not self.finished
        c = self.c
        x = np.asarray(x, dtype=np.float64)
        n = x.shape[-1]
        assert n >= 1 or final
        H = c.taps - 1
        staged = np.concatenate([self.hist, x] + ([np.zeros(x.shape[:-1] + (c.right,))] if final else []), axis=-1)
        t_end = emitted(self.n_seen + n, c.sr_in, c.sr_out, final)
        y = np.zeros(x.shape[:-1] + (max(0, t_end - self.t_next),))
        for i, t in enumerate(range(self.t_next, t_end)):
            nn, r = divmod(t * c.M, c.L)
            a0 = nn - c.left + 1 - (self.n_seen - H)                  # staged[a] = x[n_seen - H + a]
            assert a0 >= 0 and a0 + c.taps <= staged.shape[-1], (t, a0)
            self.min_first_word = min(self.min_first_word, a0)
            y[..., i] = staged[..., a0:a0 + c.taps] @ self.bank[r]
        self.hist = staged[..., n:n + H]
        self.n_seen += n
        self.t_next = max(self.t_next, t_end)
        self.finished = bool(final)
        return y


def resample_stream(x, sr_in, sr_out, chunks):
    """x (..., N) pushed in chunks of the sizes `chunks` (their sum is N; the last push is not final), then an empty final
    push.  Returns (list of the per-push outputs, the final push's included; their concatenation)."""
    x = np.asarray(x, dtype=np.float64)
    assert sum(chunks) == x.shape[-1], (sum(chunks), x.shape)
    s = Stream(sr_in, sr_out, x.shape[:-1])
    outs, at = [], 0
    for n in chunks:
        outs.append(s.push(x[..., at:at + n]))
        at += n
    outs.append(s.push(x[..., :0], final=True))
    assert s.min_first_word >= 0
    return outs, np.concatenate(outs, axis=-1)
