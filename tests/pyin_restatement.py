"""Float64 numpy / scipy restatement of the pYIN definition of DESIGN.md 3.9 (pYIN as published and as librosa structures
it; parity with librosa itself is unpinned: it is not installed where this project is built).  One function per stage; every
later stage takes the earlier stage's output, so a test can feed it the GPU's own intermediate result.  The decode keeps the
transitions banded (+ the one jump term that stands for every out-of-band transition, whose probability is 0, i.e.
log(0 + tiny)), so a 10 s clip decodes in seconds; `viterbi_dense` is the textbook form it is checked against.
"""
import math
from types import SimpleNamespace

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.stats import beta as beta_dist

N_THRESHOLDS = 100
BETA_PARAMETERS = (2, 18)
BOLTZMANN = 2.0
RESOLUTION = 0.1
MAX_TRANSITION_RATE = 35.92
SWITCH_PROB = 0.01
NO_TROUGH_PROB = 0.01
TINY32 = float(np.finfo(np.float32).tiny)      # in the cumulative-mean normalisation
TINY64 = float(np.finfo(np.float64).tiny)      # log(p + tiny) of the decode


def config(sr=16000, fmin=65.0, fmax=2093.0, frame_length=1024, hop_length=128):
    c = SimpleNamespace(sr=float(sr), fmin=float(fmin), fmax=float(fmax), frame_length=int(frame_length), hop=int(hop_length))
    c.W = c.frame_length // 2
    c.min_period = max(int(math.floor(c.sr / c.fmax)), 1)
    c.max_period = min(int(math.ceil(c.sr / c.fmin)), c.frame_length - c.W - 1)
    c.lags = c.max_period - c.min_period + 1
    c.n_bps = int(math.ceil(1.0 / RESOLUTION))
    c.n_bins = int(math.floor(12 * c.n_bps * np.log2(c.fmax / c.fmin))) + 1
    c.width = int(round(MAX_TRANSITION_RATE * 12 * c.hop / c.sr)) * c.n_bps + 1
    c.h = (c.width - 1) // 2
    assert c.width % 2 == 1
    return c


def n_frames(n, c):
    return 1 + n // c.hop


def frames(x, c, dtype=np.float64):
    """(T, frame_length): frame t = reflect-padded samples [hop t - fl/2, hop t + fl/2)"""
    x = np.asarray(x, dtype=dtype)
    xp = np.pad(x, c.frame_length // 2, mode="reflect")
    T = n_frames(x.size, c)
    return sliding_window_view(xp, c.frame_length)[::c.hop][:T]


def difference(x, c, dtype=np.float64):
    """d (T, max_period + 1): d_t(tau) = sum_{j < W} (x[j] - x[j + tau])^2, formed as squared differences in `dtype`"""
    F = frames(x, c, dtype)
    d = np.zeros((F.shape[0], c.max_period + 1), dtype=dtype)
    head = np.ascontiguousarray(F[:, :c.W])
    for tau in range(1, c.max_period + 1):
        e = head - F[:, tau:tau + c.W]
        d[:, tau] = np.sum(e * e, axis=1, dtype=dtype)
    return d


def difference_fft(x, c):
    """the same sums as energy terms - 2 x correlation, the correlation by FFT (float64): a cross-check of `difference`"""
    F = frames(x, c)
    W, P = c.W, c.max_period
    n = 1 << int(math.ceil(math.log2(c.frame_length + W)))
    a = np.fft.rfft(F[:, :W], n, axis=1)
    bb = np.fft.rfft(F, n, axis=1)
    corr = np.fft.irfft(np.conj(a) * bb, n, axis=1)[:, :P + 1]          # sum_j x[j] x[j + tau]
    cs = np.concatenate([np.zeros((F.shape[0], 1)), np.cumsum(F * F, axis=1)], axis=1)
    e_tau = cs[:, W:W + P + 1] - cs[:, 0:P + 1]                        # sum_j x[j + tau]^2
    return cs[:, W:W + 1] + e_tau - 2.0 * corr


def cmnd(d, c, dtype=np.float64):
    """yin (T, lags): d(tau) / (tiny + (1 / tau) sum_{k = 1 .. tau} d(k)) for tau in [min_period, max_period]"""
    d = np.asarray(d, dtype=dtype)
    cum = np.cumsum(d[:, 1:], axis=1, dtype=dtype)
    tau = np.arange(c.min_period, c.max_period + 1)
    mean = cum[:, tau - 1] / tau.astype(dtype)
    return (d[:, tau] / (dtype(TINY32) + mean)).astype(dtype)


def beta_masses():
    edges = np.arange(N_THRESHOLDS + 1) / 100.0
    return np.diff(beta_dist.cdf(edges, *BETA_PARAMETERS))


def observe(yin, c):
    """yin (T, lags) -> cand_bin (T, lags) int (-1 beyond count), cand_prob (T, lags), count (T), voiced_prob (T)"""
    yin = np.asarray(yin)
    T, lags = yin.shape
    assert lags == c.lags
    thetas = np.arange(1, N_THRESHOLDS + 1) / 100.0
    betas = beta_masses()
    cand_bin = np.full((T, lags), -1, dtype=np.int64)
    cand_prob = np.zeros((T, lags))
    count = np.zeros(T, dtype=np.int64)
    voiced_prob = np.zeros(T)
    for t in range(T):
        y = yin[t].astype(np.float64)
        trough = np.zeros(lags, dtype=bool)
        trough[1:-1] = (y[1:-1] < y[:-2]) & (y[1:-1] <= y[2:])
        trough[0] = y[0] < y[1]
        idx = np.nonzero(trough)[0]
        if idx.size == 0:
            continue
        hgt = y[idx]
        below = hgt[:, None] < thetas[None, :]
        m = np.cumsum(below, axis=0) - 1
        n = below.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            prior = (1 - np.exp(-BOLTZMANN)) * np.exp(-BOLTZMANN * m) / (1 - np.exp(-BOLTZMANN * n))[None, :]
            probs = np.where(below, prior * betas[None, :], 0.0).sum(axis=1)
        probs[np.argmin(hgt)] += NO_TROUGH_PROB * betas[n == 0].sum()
        a = np.zeros(lags)
        b = np.zeros(lags)
        a[1:-1] = y[:-2] + y[2:] - 2 * y[1:-1]
        b[1:-1] = (y[2:] - y[:-2]) / 2
        with np.errstate(divide="ignore", invalid="ignore"):
            shift = np.where(np.abs(b) < np.abs(a), -b / a, 0.0)
        shift[0] = shift[-1] = 0.0
        keep = probs > 0
        ci, cp = idx[keep], probs[keep]
        f0 = c.sr / (c.min_period + ci + shift[ci])
        bins = np.clip(np.rint(12 * c.n_bps * np.log2(f0 / c.fmin)), 0, c.n_bins).astype(np.int64)
        k = ci.size
        cand_bin[t, :k], cand_prob[t, :k], count[t] = bins, cp, k
        obs = np.zeros(c.n_bins + 1)
        for bn, pr in zip(bins, cp):           # assigned, not summed, in increasing lag order
            obs[bn] = pr
        voiced_prob[t] = np.clip(obs[:c.n_bins].sum(), 0, 1)
    return cand_bin, cand_prob, count, voiced_prob


def _window(c):
    k = np.arange(c.h + 1)
    return 1.0 - k / (c.h + 1.0)             # triangle of width 2 h + 1: scipy.signal.get_window("triangle", width, fftbins=False)


def _rowsum(c):
    w = _window(c)
    full = np.concatenate([w[:0:-1], w])
    return np.array([full[max(0, c.h - i):c.h + min(c.h, c.n_bins - 1 - i) + 1].sum() for i in range(c.n_bins)])


def log_observations(cand_bin, cand_prob, count, voiced_prob, c):
    """log(obs + tiny): voiced half (T, n_bins) and the common value of the unvoiced half (T,)"""
    T = len(count)
    obs = np.zeros((T, c.n_bins + 1))
    for t in range(T):
        for bn, pr in zip(cand_bin[t, :count[t]], cand_prob[t, :count[t]]):
            obs[t, bn] = pr
    return np.log(obs[:, :c.n_bins] + TINY64), np.log((1 - np.asarray(voiced_prob)) / c.n_bins + TINY64)


def transition_prob(s_from, s_to, c, rowsum=None, w=None):
    rowsum = _rowsum(c) if rowsum is None else rowsum
    w = _window(c) if w is None else w
    i, j = s_from % c.n_bins, s_to % c.n_bins
    if abs(i - j) > c.h:
        return 0.0
    same = (s_from < c.n_bins) == (s_to < c.n_bins)
    return w[abs(i - j)] / rowsum[i] * ((1 - SWITCH_PROB) if same else SWITCH_PROB)


def _log_init(c):
    return np.concatenate([np.full(c.n_bins, np.log(0.0 + TINY64)), np.full(c.n_bins, np.log(1.0 / c.n_bins + TINY64))])


def viterbi(cand_bin, cand_prob, count, voiced_prob, c):
    """-> (states (T,), log-probability of the path).  States: [voiced bins | unvoiced bins]; ties go to the lowest source state
    and to the lowest final state."""
    lv, lu = log_observations(cand_bin, cand_prob, count, voiced_prob, c)
    T, nb, h, width = len(count), c.n_bins, c.h, c.width
    w, rowsum = _window(c), _rowsum(c)
    # banded log transitions by TARGET j and offset o: source i = j + o - h
    src = np.arange(nb)[:, None] + np.arange(width)[None, :] - h
    ok = (src >= 0) & (src < nb)
    pw = np.where(ok, w[np.abs(np.arange(width) - h)][None, :] / rowsum[np.clip(src, 0, nb - 1)], 0.0)
    with np.errstate(divide="ignore"):
        lt_same = np.where(ok, np.log(pw * (1 - SWITCH_PROB) + TINY64), -np.inf)
        lt_cross = np.where(ok, np.log(pw * SWITCH_PROB + TINY64), -np.inf)
    ltiny = np.log(TINY64)
    V = _log_init(c) + np.concatenate([lv[0], np.full(nb, lu[0])])
    back = np.zeros((T, 2 * nb), dtype=np.int64)
    pad = np.full(h, -np.inf)
    for t in range(1, T):
        wv = sliding_window_view(np.concatenate([pad, V[:nb], pad]), width)
        wu = sliding_window_view(np.concatenate([pad, V[nb:], pad]), width)
        g = int(np.argmax(V))
        jump = V[g] + ltiny
        new = np.empty(2 * nb)
        for half, (la, lb) in enumerate(((lt_same, lt_cross), (lt_cross, lt_same))):
            cand = np.concatenate([wv + la, wu + lb], axis=1)          # sources in state order: voiced band, unvoiced band
            k = np.argmax(cand, axis=1)
            best = cand[np.arange(nb), k]
            source = np.where(k < width, 0, nb) + np.arange(nb) + (k % width) - h
            use_jump = jump > best
            back[t, half * nb:(half + 1) * nb] = np.where(use_jump, g, source)
            new[half * nb:(half + 1) * nb] = np.where(use_jump, jump, best)
        V = new + np.concatenate([lv[t], np.full(nb, lu[t])])
    states = np.zeros(T, dtype=np.int64)
    states[-1] = int(np.argmax(V))
    for t in range(T - 1, 0, -1):
        states[t - 1] = back[t, states[t]]
    return states, float(V[states[-1]])


def viterbi_dense(cand_bin, cand_prob, count, voiced_prob, c):
    """the textbook decode over the full (2 n_bins)^2 matrix of log(p + tiny): for short clips"""
    lv, lu = log_observations(cand_bin, cand_prob, count, voiced_prob, c)
    T, nb = len(count), c.n_bins
    w, rowsum = _window(c), _rowsum(c)
    i, j = np.arange(nb)[:, None], np.arange(nb)[None, :]
    band = np.where(np.abs(i - j) <= c.h, w[np.minimum(np.abs(i - j), c.h)] / rowsum[:, None], 0.0)
    P = np.block([[band * (1 - SWITCH_PROB), band * SWITCH_PROB], [band * SWITCH_PROB, band * (1 - SWITCH_PROB)]])
    LT = np.log(P + TINY64)
    V = _log_init(c) + np.concatenate([lv[0], np.full(nb, lu[0])])
    back = np.zeros((T, 2 * nb), dtype=np.int64)
    for t in range(1, T):
        M = V[:, None] + LT
        back[t] = np.argmax(M, axis=0)
        V = M[back[t], np.arange(2 * nb)] + np.concatenate([lv[t], np.full(nb, lu[t])])
    states = np.zeros(T, dtype=np.int64)
    states[-1] = int(np.argmax(V))
    for t in range(T - 1, 0, -1):
        states[t - 1] = back[t, states[t]]
    return states, float(V[states[-1]])


def path_log_probability(states, cand_bin, cand_prob, count, voiced_prob, c):
    """log-probability of ANY state path under this model, in float64"""
    lv, lu = log_observations(cand_bin, cand_prob, count, voiced_prob, c)
    w, rowsum = _window(c), _rowsum(c)
    states = np.asarray(states, dtype=np.int64)
    obs = lambda t, s: lv[t, s] if s < c.n_bins else lu[t]
    total = _log_init(c)[states[0]] + obs(0, states[0])
    for t in range(1, len(states)):
        total += np.log(transition_prob(states[t - 1], states[t], c, rowsum, w) + TINY64) + obs(t, states[t])
    return float(total)


def decode(states, c, fill_na=None):
    """-> (f0, voiced flag): f0 = fmin 2^(bin / (12 n_bps)); fill_na=None keeps it on unvoiced frames"""
    states = np.asarray(states, dtype=np.int64)
    voiced = states < c.n_bins
    f0 = c.fmin * 2.0 ** ((states % c.n_bins) / (12.0 * c.n_bps))
    if fill_na is not None:
        f0 = np.where(voiced, f0, fill_na)
    return f0, voiced


def pyin(x, c, dtype=np.float64):
    """every stage from audio; `dtype` is the precision of the difference function and its normalisation only"""
    r = SimpleNamespace()
    r.yin = cmnd(difference(x, c, dtype), c, dtype)
    r.cand_bin, r.cand_prob, r.count, r.voiced_prob = observe(r.yin, c)
    r.states, r.logp = viterbi(r.cand_bin, r.cand_prob, r.count, r.voiced_prob, c)
    r.f0, r.voiced = decode(r.states, c)
    return r
