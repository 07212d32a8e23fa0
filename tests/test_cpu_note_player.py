"""CPU tests of the note player: properties of the float64 restatement (tests/note_control_restatement.py), the
float32 yardstick the GPU tests' bar is built from (and that the bar trips on a float32 phase product), the host-side scheduling
of streaming.NoteBook, the refusals of the two C entry points that need no device, and the surface."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import note_control_restatement as nc
from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"
FLOOR_L, FLOOR_F0 = 1e-6, 2e-6          # the floors of the GPU tests' bar: loudness units, relative F0


def _streaming():
    return importlib.import_module(PKG + ".streaming")


def _lib():
    return importlib.import_module(PKG + "._lib")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_envelope_hits_its_corners_exactly(dtype):
    P = nc.params(attack=3, decay=4, release=5)
    v, j_off = 0.7, 11
    p = dtype(P["peak_lo"]) + dtype(v) * (dtype(P["peak_hi"]) - dtype(P["peak_lo"]))
    l = nc.loudness(np.arange(40), v, j_off, P, dtype)
    assert l[2] == p                                          # the attack ends on p at j = A - 1
    assert l[6] == p - dtype(P["drop"])                       # the decay ends on p - drop at j = A + D - 1
    assert np.all(l[7:j_off] == p - dtype(P["drop"]))         # sustain
    assert np.all(np.diff(l[:3]) > 0) and np.all(np.diff(l[2:7]) < 0) and np.all(np.diff(l[j_off - 1:j_off + 5]) < 0)
    assert l[j_off + 4] == dtype(P["silence"]) and np.all(l[j_off + 4:] == dtype(P["silence"]))    # q exactly at j_off + R - 1, and after
    assert l[j_off + 3] > dtype(P["silence"])
    # the definition's own form of the attack and the release, to rounding
    q = P["silence"]
    assert abs(float(l[0]) - (q + (float(p) - q) * 1 / 3)) < 1e-6
    h_off = float(l[j_off - 1])
    assert abs(float(l[j_off + 1]) - (h_off + (q - h_off) * 2 / 5)) < 1e-6


def test_release_inside_attack_and_decay_starts_from_the_level_reached():
    P = nc.params(attack=6, decay=4, release=3)
    for j_off in (2, 8):
        held = nc.loudness(np.arange(20), 0.5, nc.HELD, P)
        l = nc.loudness(np.arange(20), 0.5, j_off, P)
        assert np.array_equal(l[:j_off], held[:j_off])
        h_off, q = held[j_off - 1], P["silence"]
        assert np.allclose(l[j_off:j_off + 3], [q + (h_off - q) * 2 / 3, q + (h_off - q) / 3, q], rtol=0, atol=1e-15)


def test_degenerate_envelopes_are_well_defined():
    for A, D in ((0, 4), (3, 0), (0, 0)):
        P = nc.params(attack=A, decay=D, release=2)
        f0, control, l = nc.note(np.arange(12), 60.0, 1.0, nc.HELD, P)
        assert np.isfinite(f0).all() and np.isfinite(control).all()
        assert l[A + D] == P["peak_hi"] - P["drop"]
        if A == 0 and D > 0:
            assert l[0] == P["peak_hi"] - P["drop"] * (1 / 4)        # no attack: the first frame is the decay's first
        if A == 0 and D == 0:
            assert np.all(l == P["peak_hi"] - P["drop"])
    # j_off = 0: the voice never leaves silence's ramp: h_off = h(-1) = q, so every frame is q
    P = nc.params(release=4)
    l = nc.loudness(np.arange(8), 0.9, 0, P)
    assert np.all(l == P["silence"])
    # R = 1: the first release frame is already q
    l = nc.loudness(np.arange(12), 0.9, 9, nc.params(release=1))
    assert l[8] > P["silence"] and l[9] == P["silence"]


def test_vibrato_is_exactly_zero_through_its_delay_and_bounded_after():
    P = nc.params(vib_delay=6, vib_ramp=10, vib_depth=40.0)
    for dtype in (np.float64, np.float32):
        j = np.arange(200)
        c = nc.vibrato_cents(j, P, dtype)
        assert np.all(c[:7] == 0) and c[8] != 0
        f0 = nc.note(j, 57.0, 0.5, nc.HELD, P, dtype)[0]
        assert np.all(f0[:7] == dtype(220.0))                                     # A3, untouched
        assert np.abs(c).max() <= 40.0 and np.abs(c[16:]).max() > 39.0
        assert np.abs(c[:17]).max() <= 40.0 * (np.arange(17) - 6).clip(0, 10).max() / 10
    # equal temperament
    assert nc.note(np.arange(1), 69.0, 0.5, nc.HELD, P)[0][0] == 440.0
    assert abs(nc.note(np.arange(1), 81.0, 0.5, nc.HELD, P)[0][0] - 880.0) < 1e-10


def test_control_channels_are_the_normalised_features():
    P = nc.params()
    f0, control, l = nc.note(np.arange(30), 64.0, 0.6, 20, P)
    assert np.allclose(control[0] * P["std0"] + P["mean0"], f0, rtol=1e-14)
    assert np.allclose(control[1] * P["std1"] + P["mean1"], l, rtol=1e-14)


def test_float32_with_an_exact_phase_stays_inside_the_floors_over_a_long_note():
    """A, D, R = 3, 4, 5, 5.5 Hz, 40 cents, 40 000 frames: measured 5.2e-8 loudness units and 2.9e-7 relative F0 here."""
    P = nc.params(attack=3, decay=4, release=5, vib_rate=5.5, vib_depth=40.0)
    j = np.arange(40000)
    for j_off in (nc.HELD, 39990):
        f64, _, l64 = nc.note(j, 64.3, 0.7, j_off, P)
        f32, _, l32 = nc.note(j, 64.3, 0.7, j_off, P, np.float32)
        e_l, e_f = np.abs(l32 - l64).max(), (np.abs(f32 - f64) / f64).max()
        print("float32 restatement vs float64:", e_l, e_f)
        assert e_l <= FLOOR_L and e_f <= FLOOR_F0
        # ... and its error does not grow with j
        assert (np.abs(f32 - f64) / f64)[-4000:].max() <= 2.0 * (np.abs(f32 - f64) / f64)[:4000].max()


def test_a_float32_phase_product_is_outside_them():
    """the same note with the phase formed in float32: 8.4e-6 relative here - a kernel that formed it so would miss the GPU tests' bar"""
    P = nc.params(attack=3, decay=4, release=5, vib_rate=5.5, vib_depth=40.0)
    j = np.arange(40000)
    f64 = nc.note(j, 64.3, 0.7, nc.HELD, P)[0]
    f32 = nc.note(j, 64.3, 0.7, nc.HELD, P, np.float32, phase="product")[0]
    e = np.abs(f32 - f64) / f64
    print("float32 phase product vs float64:", e.max())
    assert e.max() > FLOOR_F0 and e[-4000:].max() > 4.0 * e[:4000].max()


def test_hop_by_hop_control_does_not_depend_on_the_hop_size():
    P = nc.params()
    runs = []
    for K in (1, 2, 16):
        s = nc.Control(2, P)
        f0s, controls = [], []
        for h in range(32 // K):
            a = h * K
            if a == 0:
                s.notes[0] = (60.0, 0.8, nc.HELD)
            if a == 16:
                s.notes[1] = (67.0, 0.4, nc.HELD)
                s.notes[0] = (60.0, 0.8, 16)
            words = [nc.ACTIVE | (nc.START if a == 0 else 0), 0 if a < 16 else nc.ACTIVE | (nc.START if a == 16 else 0)]
            f0, control = s.hop(words, K)
            f0s.append(f0)
            controls.append(control)
        runs.append((np.concatenate(f0s, axis=1), np.concatenate(controls, axis=2)))
    for f0, control in runs[1:]:
        assert np.array_equal(f0, runs[0][0]) and np.array_equal(control, runs[0][1])
    f0, control = runs[0]
    assert not f0[1, :16].any() and not control[1, :, :16].any() and f0[1, 16:].all()
    assert np.array_equal(f0[1, 16:], nc.note(np.arange(16), 67.0, 0.4, nc.HELD, P)[0])
    assert np.array_equal(control[0], nc.note(np.arange(32), 60.0, 0.8, 16, P)[1])


def test_voice_mix_and_pan():
    rng = np.random.default_rng(0)
    o, g = rng.standard_normal((3, 7)), rng.standard_normal((3, 2))
    out, scale = nc.voice_mix(o, g)
    assert out.shape == (2, 7) and np.allclose(out, g.T @ o) and np.all(scale >= np.abs(out))
    for pan in (-1.0, -0.3, 0.0, 1.0):
        l, r = nc.pan_gains(pan, 2)
        assert abs(l * l + r * r - 1.0) < 1e-15
        assert np.allclose(_streaming().pan_gains(pan, 2), (l, r), rtol=0, atol=1e-15)
    assert np.allclose(nc.pan_gains(-1.0, 2), (1.0, 0.0), atol=1e-15) and np.allclose(nc.pan_gains(1.0, 2), (0.0, 1.0), atol=1e-15)
    assert nc.pan_gains(0.3, 1) == (1.0,) == _streaming().pan_gains(0.3, 1)
    with pytest.raises(RuntimeError):
        _streaming().pan_gains(1.5, 2)


# ---- NoteBook -------------------------------------------------------------------------------------------------------------------
def _hop(book):
    start, stop = book.plan()
    book.commit()
    return start, stop


def test_notebook_allocates_the_lowest_idle_slot_and_counts_drops():
    s = _streaming()
    book = s.NoteBook(3, 2, 4)
    a, b, c = book.note_on(60), book.note_on(62), book.note_on(64)
    assert (a, b, c) == (0, 1, 2) and book.active() == [0, 1, 2]
    assert book.note_on(65) is None and book.note_on(66) is None and book.dropped == 2
    assert _hop(book) == ([0, 1, 2], [])
    assert [n[0] for n in book.notes] == [60.0, 62.0, 64.0] and all(n[2] == s.NOTE_HELD for n in book.notes)
    assert book.note_on(65) is None and book.dropped == 3
    book.note_off(b)                     # slot 1: j_off = 2, stop on the hop with frame 5: voice hop 2
    assert _hop(book) == ([], []) and book.notes[1][2] == 2 and book.stop_hop(b) == 2 and book.stop_hop(a) is None
    assert _hop(book) == ([], [1])
    assert book.slots.states == ["active", "releasing", "active"] and book.active() == [0, 2]
    assert book.note_on(70) is None and book.dropped == 4          # a slot in its release hop is not handed out
    assert _hop(book) == ([], [])
    d = book.note_on(70)
    assert d == 3 and book._slot_of[d] == 1                        # the freed slot, the only idle one
    assert book.note_on(71) is None                                # taken by the queued note-on
    assert _hop(book) == ([1], [])
    assert book.notes[1] == (70.0, 0.8, s.NOTE_HELD) and book.frames == [10, 2, 10]


@pytest.mark.parametrize("K, R, hops_after_off", [(4, 2, 0), (4, 4, 0), (4, 5, 1), (4, 9, 2), (1, 3, 2), (16, 5, 0), (2, 25, 12)])
def test_notebook_puts_the_stop_on_the_hop_with_the_last_release_frame(K, R, hops_after_off):
    """R < K, R = K, R no multiple of K: the stop hop contains frame j_off + R - 1, and every frame of it belongs to the voice"""
    book = _streaming().NoteBook(2, K, R)
    h = book.note_on(60)
    for _ in range(3):
        _hop(book)
    book.note_off(h)
    stops = []
    for i in range(hops_after_off + 3):
        start, stop = _hop(book)
        stops.append(stop)
    assert book.notes[0][2] == 3 * K
    assert stops.index([0]) == hops_after_off == (3 * K + R - 1) // K - 3
    assert all(s == [] for i, s in enumerate(stops) if i != hops_after_off)
    assert book.slots.states[0] == "idle" and book.active() == []
    assert book.frames[0] == (3 + hops_after_off + 1) * K


def test_notebook_note_on_and_off_between_the_same_two_hops():
    s = _streaming()
    for K, R, n_hops in ((4, 3, 1), (4, 4, 1), (4, 6, 2), (1, 2, 2)):
        book = s.NoteBook(2, K, R)
        h = book.note_on(60, 0.5)
        book.note_off(h)
        book.note_off(h)                                           # twice: the second is ignored
        seen = [_hop(book) for _ in range(n_hops + 2)]
        assert book.notes[0] == (60.0, 0.5, 0)                     # released before its first hop: j_off = 0
        assert seen[0][0] == [0] and [x[1] for x in seen].index([0]) == n_hops - 1 == (R - 1) // K
        assert book.slots.states == ["idle", "idle"]
    book = s.NoteBook(1, 2, 2)
    book.note_off(None)
    book.note_off(17)                                              # unknown handles are ignored
    assert _hop(book) == ([], [])
    with pytest.raises(RuntimeError):
        book.note_on(60, 0.0)
    with pytest.raises(RuntimeError):
        book.note_on(60, 1.5)
    with pytest.raises(RuntimeError):
        s.NoteBook(1, 17, 2)
    with pytest.raises(RuntimeError):
        s.NoteBook(1, 2, 0)


def test_notebook_words_drive_the_restatement_like_a_single_note():
    """the book's events through the hop-by-hop restatement = the closed form of each note, whatever the hop size"""
    s = _streaming()
    P = nc.params(release=5)
    for K in (1, 2, 16):
        book, ctl = s.NoteBook(2, K, 5), nc.Control(2, P)
        f0s, words_seen = [], []
        for hop in range(48 // K):
            if hop * K == 16:
                h = book.note_on(72.0, 0.9)
            if hop * K == 32:
                book.note_off(h)
            start, stop = book.plan()
            words = list(book._planned)
            ctl.notes = list(book.notes)
            f0s.append(ctl.hop(words, K)[1][0, 1])
            words_seen.append(words[0])
            book.commit()
        got = np.concatenate(f0s)
        want = (nc.loudness(np.arange(32), 0.9, 16, P) - P["mean1"]) / P["std1"]
        n = (16 + 5 - 1) // K * K + K                              # frames through the stop hop
        assert np.array_equal(got[16:16 + n], want[:n]) and not got[:16].any() and not got[16 + n:].any()
        assert want[20] == (P["silence"] - P["mean1"]) / P["std1"]


# ---- the C entry points: refusals that need no device ---------------------------------------------------------------------------------
def _player(**kw):
    L = _lib()
    P = L.NwsNotePlayer()
    for k, v in nc.params(**kw).items():
        if k in ("mean0", "mean1"):
            P.mean[int(k[-1])] = v
        elif k in ("std0", "std1"):
            P.std[int(k[-1])] = v
        else:
            setattr(P, k, int(v) if k in ("attack", "decay", "release", "vib_delay", "vib_ramp") else v)
    return P


def test_refusals_come_before_any_launch_and_touch_nothing():
    """no GPU here: a call that got as far as the runtime would return a HIP error code (positive), never -1 / -2"""
    L = _lib().lib()
    assert [L.nws_note_control_state_bytes(B) for B in (0, -1, 65536)] == [0, 0, 0]
    assert L.nws_note_control_state_bytes(1) >= 4 and L.nws_note_control_state_bytes(65535) >= 4 * 65535
    buf = np.full(1 << 16, 7.0, dtype=np.float32)                   # poisoned: every pointer of the calls below
    p, nbytes = buf.ctypes.data, buf.nbytes
    assert L.nws_note_control_reset(None, nbytes, 2, None) == -2 and L.nws_note_control_reset(p, nbytes, 0, None) == -2
    assert L.nws_note_control_reset(p, L.nws_note_control_state_bytes(5) - 1, 5, None) == -2
    assert L.nws_note_control_reset(p, nbytes, 65536, None) == -1

    def control(player=None, ev=p, notes=p, state=p, size=nbytes, B=5, K=2, f0=p, ctl=p, **kw):
        P = _player(**kw) if player is None else player
        return L.nws_note_control(C.byref(P) if P is not False else None, ev, notes, state, size, B, K, f0, ctl, None)

    assert control(player=False) == -2 and control(ev=None) == -2 and control(notes=None) == -2 and control(state=None) == -2
    assert control(f0=None) == -2 and control(ctl=None) == -2
    assert control(B=0) == -2 and control(K=0) == -2 and control(K=17) == -2 and control(K=-1) == -2
    assert control(release=0) == -2 and control(vib_ramp=0) == -2 and control(attack=-1) == -2 and control(decay=-1) == -2
    assert control(vib_delay=-1) == -2 and control(attack=(1 << 24) + 1) == -2
    assert control(std0=0.0) == -2 and control(std1=-1.0) == -2 and control(sample_rate=0.0) == -2 and control(drop=-0.1) == -2
    assert control(std0=float("nan")) == -2 and control(vib_rate=-1.0) == -2
    assert control(size=L.nws_note_control_state_bytes(5) - 1) == -2
    assert control(B=65536) == -1

    def mix(o=p, gain=p, B=3, N=128, Cn=1, out=p):
        return L.nws_voice_mix(o, gain, B, N, Cn, out, None)

    assert mix(o=None) == -2 and mix(gain=None) == -2 and mix(out=None) == -2
    assert mix(B=0) == -2 and mix(N=0) == -2 and mix(N=-4) == -2 and mix(Cn=0) == -2 and mix(Cn=3) == -2
    assert mix(B=65536) == -1 and mix(B=65536, Cn=2) == -1
    assert np.all(buf == 7.0)                                       # nothing wrote the buffer


# ---- surface --------------------------------------------------------------------------------------------------------------------
def test_symbols_in_the_header_and_both_bindings():
    with open(os.path.join(ROOT, "include", "nws_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define NWS_ABI_VERSION 6\b", header)
    lib_mod = _lib()
    for name in ("nws_note_control_state_bytes", "nws_note_control_reset", "nws_note_control", "nws_voice_mix"):
        assert re.search(r"\b" + name + r"\(", header) and name in lib_mod.EXPORTED_SYMBOLS
        assert getattr(lib_mod.lib(), name).argtypes is not None
    with open(os.path.join(ROOT, PKG, "csrc", "torch_ops.cpp")) as f:
        ops = f.read()
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    for op in ("note_control_reset", "note_control", "voice_mix"):
        assert re.search(r'm\.def\("' + op + r"\(", ops) and callable(getattr(cops, op)), op
    assert lib_mod.NOTE_PARAMS == nc.PARAMS and lib_mod.NOTE_HELD == nc.HELD
    # the ctypes struct has the header's fields in the header's order
    body = re.search(r"typedef struct NwsNotePlayer \{(.*?)\} NwsNotePlayer;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [n for n, _ in lib_mod.NwsNotePlayer._fields_]
    assert C.sizeof(lib_mod.NwsNotePlayer) == 72


def test_player_surface():
    s = _streaming()
    sig = inspect.signature(s.NotePlayer.__init__)
    names = list(sig.parameters)
    assert names[:5] == ["self", "model", "voices", "hop_frames", "channels"]
    assert sig.parameters["hop_frames"].default == 1 and sig.parameters["channels"].default == 1
    kw = {n for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert kw == {"attack", "decay", "release", "drop", "silence", "peak_lo", "peak_hi", "vib_rate", "vib_depth", "vib_delay", "vib_ramp",
                  "normalisation", "phase_u", "noise", "graph"}
    for name, params in (("note_on", ["self", "pitch", "velocity", "pan"]), ("note_off", ["self", "handle"]), ("hop", ["self"]),
                         ("render", ["self", "n_hops"]), ("active", ["self"]), ("check", ["self"]), ("close", ["self"])):
        assert list(inspect.signature(getattr(s.NotePlayer, name)).parameters) == params, name
    on = inspect.signature(s.NotePlayer.note_on).parameters
    assert on["velocity"].default == 0.8 and on["pan"].default == 0.0
    assert "nobody has listened" in s.NotePlayer.__doc__
    model_cls = importlib.import_module(PKG).NeuralWaveshaping
    assert list(inspect.signature(model_cls.player).parameters)[:2] == ["self", "voices"]
    for script in ("play_score.py", "time_player.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", script))
