"""Restatement of the note player's definition in numpy: the frame-rate controls of one held and released note
as closed forms in the voice's frame index j, the same controls hop by hop for B slots under event words (what nws_note_control
computes), and the voice mix.  float64 is the definition the kernels are held near; dtype=np.float32 is the yardstick - the same
arithmetic in the kernels' precision, with the vibrato phase still formed and reduced exactly (in float64), or, with
phase="product", as a float32 product (which loses the phase over a long note, and is there to show that the tests' bar trips).

Frames are control frames of 128 samples.  Per voice: pitch (MIDI note number), velocity v in (0, 1], j_off (first release frame,
HELD while the note is held).  Per player: P, a dict with the keys of PARAMS.

    p     = lo + v (hi - lo)
    h(j)  = q + (p - q) (j + 1) / A          j < A
            p - drop (j - A + 1) / D         A <= j < A + D
            p - drop                         otherwise;     h(-1) := q
    l(j)  = h(j)                                            j < j_off
            h_off + (q - h_off) min(j - j_off + 1, R) / R   j >= j_off,   h_off = h(j_off - 1)
    r(j)  = clamp((j - delay) / ramp, 0, 1)
    c(j)  = depth r(j) sin(2 pi frac(rate 128 j / sr))
    f0(j) = 440 2^((pitch - 69) / 12 + c(j) / 1200)
    control(j) = ((f0(j) - mean0) / std0, (l(j) - mean1) / std1)

The attack and the release are evaluated from the end they have to hit,
    q + (p - q) (j + 1) / A = p - (p - q) (A - 1 - j) / A,      h_off + (q - h_off) m / R = q + (h_off - q) (R - m) / R,
so that h(A - 1) is p and l(j_off + R - 1) is q bit for bit in any precision."""
import numpy as np

HELD = 2 ** 31 - 1
HOP = 128
START, STOP, RELEASE, ACTIVE = 1, 2, 4, 8      # include/nws_hip.h NWS_SLOT_*
PARAMS = ("attack", "decay", "release", "vib_delay", "vib_ramp", "drop", "silence", "peak_lo", "peak_hi", "vib_rate", "vib_depth",
          "sample_rate", "mean0", "std0", "mean1", "std1")


def params(attack=3, decay=4, release=5, vib_delay=6, vib_ramp=10, drop=0.1, silence=0.2, peak_lo=0.5, peak_hi=0.9, vib_rate=5.5,
           vib_depth=40.0, sample_rate=16000.0, mean0=300.0, std0=150.0, mean1=0.6, std1=0.15):
    return dict(zip(PARAMS, (attack, decay, release, vib_delay, vib_ramp, drop, silence, peak_lo, peak_hi, vib_rate, vib_depth,
                             sample_rate, mean0, std0, mean1, std1)))


def held_level(j, p, P, dtype=np.float64):
    """h(j) for an array of frame indices j >= -1"""
    j = np.asarray(j, dtype=np.int64)
    A, D = int(P["attack"]), int(P["decay"])
    q, drop = dtype(P["silence"]), dtype(P["drop"])
    p = dtype(p)
    out = np.full(j.shape, p - drop, dtype=dtype)
    if A > 0:
        att = (j >= 0) & (j < A)
        out[att] = p - (p - q) * ((A - 1 - j[att]).astype(dtype) / dtype(A))
    if D > 0:
        dec = (j >= A) & (j < A + D)
        out[dec] = p - drop * ((j[dec] - A + 1).astype(dtype) / dtype(D))
    out[j < 0] = q
    return out


def loudness(j, velocity, j_off, P, dtype=np.float64):
    """l(j) for an array of frame indices j >= 0"""
    j = np.asarray(j, dtype=np.int64)
    R, q = int(P["release"]), dtype(P["silence"])
    p = dtype(P["peak_lo"]) + dtype(velocity) * (dtype(P["peak_hi"]) - dtype(P["peak_lo"]))
    out = held_level(j, p, P, dtype)
    rel = j >= j_off
    if rel.any():
        h_off = held_level(np.array([j_off - 1]), p, P, dtype)[0]
        m = np.minimum(j[rel] - j_off + 1, R)
        out[rel] = q + (h_off - q) * ((R - m).astype(dtype) / dtype(R))
    return out


def vibrato_cents(j, P, dtype=np.float64, phase="exact"):
    """c(j).  phase="exact": rate 128 j / sr formed and reduced in float64 whatever the dtype; "product": formed in dtype"""
    j = np.asarray(j, dtype=np.int64)
    r = np.clip((j - int(P["vib_delay"])).astype(dtype) / dtype(P["vib_ramp"]), dtype(0), dtype(1))
    if phase == "exact":
        turns = np.float64(P["vib_rate"]) * np.float64(HOP) * j.astype(np.float64) / np.float64(P["sample_rate"])
        frac = (turns - np.floor(turns)).astype(dtype)
    else:
        turns = dtype(P["vib_rate"]) * dtype(HOP) * j.astype(dtype) / dtype(P["sample_rate"])
        frac = turns - np.floor(turns)
    return dtype(P["vib_depth"]) * r * np.sin(dtype(2.0 * np.pi) * frac).astype(dtype)


def note(j, pitch, velocity, j_off, P, dtype=np.float64, phase="exact"):
    """frames j of one voice -> (f0 (n,), control (2, n), loudness (n,)) in dtype"""
    l = loudness(j, velocity, j_off, P, dtype)
    c = vibrato_cents(j, P, dtype, phase)
    f0 = (dtype(440.0) * np.exp2((dtype(pitch) - dtype(69.0)) / dtype(12.0) + c / dtype(1200.0))).astype(dtype)
    control = np.stack([(f0 - dtype(P["mean0"])) / dtype(P["std0"]), (l - dtype(P["mean1"])) / dtype(P["std1"])])
    return f0, control.astype(dtype), l


class Control:
    """nws_note_control hop by hop: B slots, the per-slot frame counter, the note table the host writes"""

    def __init__(self, B, P, dtype=np.float64):
        self.B, self.P, self.dtype = B, P, dtype
        self.counter = np.zeros(B, dtype=np.int64)
        self.notes = [(0.0, 0.0, HELD)] * B          # (pitch, velocity, j_off) per slot

    def hop(self, words, K):
        """the hop's event words (B) -> (f0 (B, K), control (B, 2, K)); idle and releasing slots are 0"""
        f0 = np.zeros((self.B, K), dtype=self.dtype)
        control = np.zeros((self.B, 2, K), dtype=self.dtype)
        for b, w in enumerate(words):
            if not w & ACTIVE:
                continue
            j0 = 0 if w & START else int(self.counter[b])
            pitch, velocity, j_off = self.notes[b]
            f0[b], control[b], _ = note(np.arange(j0, j0 + K), pitch, velocity, j_off, self.P, self.dtype)
            self.counter[b] = j0 + K
        return f0, control


def voice_mix(o, gain):
    """out[c, n] = sum_b gain[b, c] o[b, n] in float64, and the sum of the terms' magnitudes (the scale of a rounding bound)"""
    o, gain = np.asarray(o, dtype=np.float64), np.asarray(gain, dtype=np.float64)
    terms = gain.T[:, :, None] * o[None, :, :]        # (C, B, N)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def pan_gains(pan, channels):
    """constant-power law: pan in [-1, 1] -> (left, right) = (cos, sin) of (pan + 1) pi / 4; one channel: gain 1"""
    if channels == 1:
        return (1.0,)
    a = (float(pan) + 1.0) * np.pi / 4.0
    return (float(np.cos(a)), float(np.sin(a)))
