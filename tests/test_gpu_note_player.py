"""-m gpu tests of the note player: nws_note_control against the float64 restatement of
tests/note_control_restatement.py under a bar built from the float32 restatement's own distance, its independence of the hop size,
a note held for 40 000 frames, nws_voice_mix, streaming.NotePlayer end to end against a VoiceStream driven by hand, scripts/play_score.py,
the refusals on the device, and the file once more through the ctypes binding."""
import importlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import note_control_restatement as nc
from conftest import ROOT, load_npz, rms
from gpu_util import build_model, record

pytestmark = pytest.mark.gpu

PKG = "neural-waveshaping-synthesis_amd"
P = nc.params(attack=3, decay=4, release=5, vib_delay=6, vib_ramp=10)
FRAMES, B = 48, 5
FLOOR_L, FLOOR_F0 = 1e-6, 2e-6            # loudness units, relative F0
CAP_L, CAP_F0 = 1.25e-4, 5.8e-5           # 0.01 dB, 0.1 cent: below what can be heard
# slot -> (first frame, pitch, velocity, j_off, the frame at which the host writes j_off into the table) or None
VOICES = {0: None,                                   # never used
          1: (0, 57.0, 0.9, nc.HELD, None),          # starts at frame 0, held to the end
          2: (16, 64.5, 0.35, 5, 16),                # starts later, released in its decay (known at its start)
          3: (16, 71.0, 0.6, 16, 32),                # released in its sustain: the table row changes while the voice sounds
          4: (32, 45.25, 1.0, 3, 32)}                # starts and ends in one hop at K = 16
CASES = {0: "unused", 1: "from_frame_0", 2: "released_in_decay", 3: "released_in_sustain", 4: "one_hop_at_K16"}


def ops():
    return importlib.import_module(PKG + ".engine").binding()


def lib():
    return importlib.import_module(PKG + "._lib").lib()


def params_tensor(p):
    return torch.tensor([float(p[k]) for k in nc.PARAMS], dtype=torch.float64)


def notes_tensor(notes):
    t = np.zeros((len(notes), 4), dtype=np.int32)
    t[:, 0] = np.array([n[0] for n in notes], dtype=np.float32).view(np.int32)
    t[:, 1] = np.array([n[1] for n in notes], dtype=np.float32).view(np.int32)
    t[:, 2] = [n[2] for n in notes]
    return torch.from_numpy(t).cuda()


def new_state(n_slots):
    state = torch.empty(lib().nws_note_control_state_bytes(n_slots), dtype=torch.uint8, device="cuda")
    ops().note_control_reset(state, n_slots)
    return state


def schedule(K):
    """per hop: (event words, the note table as of this hop) for VOICES cut into hops of K frames"""
    hops, notes = [], [(0.0, 0.0, nc.HELD)] * B
    stopped = {}
    for h in range(FRAMES // K):
        a, words = h * K, []
        for b in range(B):
            v = VOICES[b]
            w = 0
            if v is not None and a + K > v[0] and b not in stopped:
                first, pitch, velocity, j_off, at = v
                if a <= first < a + K:
                    notes = notes[:b] + [(pitch, velocity, j_off if at == first else nc.HELD)] + notes[b + 1:]
                    w |= nc.START
                if at is not None and a <= at < a + K:
                    notes = notes[:b] + [(pitch, velocity, j_off)] + notes[b + 1:]
                w |= nc.ACTIVE
                if j_off != nc.HELD and a <= first + j_off + P["release"] - 1 < a + K:
                    w |= nc.STOP
                    stopped[b] = h
            elif stopped.get(b) == h - 1:
                w = nc.RELEASE
            words.append(w)
        hops.append((words, list(notes)))
    return hops


def run_kernel(K):
    """VOICES through nws_note_control in hops of K frames -> f0 (B, FRAMES), control (B, 2, FRAMES), active (B, FRAMES) bool"""
    state, params = new_state(B), params_tensor(P)
    f0s, controls, active = [], [], []
    for words, notes in schedule(K):
        f0 = torch.full((B, K), 7.0, device="cuda")
        control = torch.full((B, 2, K), 7.0, device="cuda")
        ops().note_control(params, torch.tensor(words, dtype=torch.int32).cuda(), notes_tensor(notes), state, f0, control)
        f0s.append(f0)
        controls.append(control)
        active.append(torch.tensor([bool(w & nc.ACTIVE) for w in words]).unsqueeze(1).expand(B, K))
    return torch.cat(f0s, 1).cpu(), torch.cat(controls, 2).cpu(), torch.cat(active, 1)


def run_restatement(K, dtype):
    ctl = nc.Control(B, P, dtype)
    f0s, controls = [], []
    for words, notes in schedule(K):
        ctl.notes = notes
        f0, control = ctl.hop(words, K)
        f0s.append(f0)
        controls.append(control)
    return np.concatenate(f0s, 1), np.concatenate(controls, 2)


@pytest.fixture(scope="module")
def runs():
    return {K: run_kernel(K) for K in (1, 2, 16)}


def distances(f0, control, f0_64, control_64, p, sel):
    """(loudness units, relative F0, relative F0 seen through its normalised channel) over the frames `sel`"""
    if not sel.any():
        return 0.0, 0.0, 0.0
    d_l = float(np.abs(control[1] - control_64[1])[sel].max()) * p["std1"]
    d_f = float((np.abs(f0 - f0_64) / np.where(sel, f0_64, 1.0))[sel].max())
    d_c = float((np.abs(control[0] - control_64[0]) * p["std0"] / np.where(sel, f0_64, 1.0))[sel].max())
    return d_l, d_f, d_c


def bars(yard):
    """per tensor: max(10 x yardstick, floor), never above what can be heard; the normalised channels are judged in the units of
    the features they normalise (their error times std), so they are held to these errors divided by std"""
    y_l, y_f, y_c = yard
    return min(max(10 * y_l, FLOOR_L), CAP_L), min(max(10 * y_f, FLOOR_F0), CAP_F0), min(max(10 * y_c, FLOOR_F0), CAP_F0)


# ---- (a) the control op against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 16])
def test_control_op_against_the_restatement(runs, K):
    f0, control, active = (t.numpy() for t in runs[K])
    f0_64, control_64 = run_restatement(K, np.float64)
    f0_32, control_32 = run_restatement(K, np.float32)
    assert not f0[~active].any() and not control[:, 0][~active].any() and not control[:, 1][~active].any()    # idle, releasing: exactly 0
    assert not active[0].any() and active[1].all() and active[4, 32:40].all() and not active[4, :32].any()
    assert np.isfinite(f0).all() and np.isfinite(control).all()
    for b in range(B):
        sel = active[b]
        d = distances(f0[b], control[b], f0_64[b], control_64[b], P, sel)
        yard = distances(f0_32[b].astype(np.float64), control_32[b].astype(np.float64), f0_64[b], control_64[b], P, sel)
        bar = bars(yard)
        record(f"note_control_K{K}_{CASES[b]}", loudness_err=d[0], loudness_yardstick=yard[0], loudness_ratio=d[0] / max(yard[0], 1e-30),
               f0_rel_err=d[1], f0_rel_yardstick=yard[1], f0_ratio=d[1] / max(yard[1], 1e-30), control0_rel_err=d[2],
               control0_rel_yardstick=yard[2], frames=int(sel.sum()))
        print(f"K {K} {CASES[b]}: kernel {d}, yardstick {yard}, bar {bar}")
        assert d[0] <= bar[0] and d[1] <= bar[1] and d[2] <= bar[2], (CASES[b], d, yard, bar)
    # the envelope's corners, bit for bit: the held note's last attack frame is p, its sustain p - drop; a release ends on q
    p1 = np.float32(P["peak_lo"]) + np.float32(0.9) * (np.float32(P["peak_hi"]) - np.float32(P["peak_lo"]))
    level = lambda x: np.float32((np.float32(x) - np.float32(P["mean1"])) / np.float32(P["std1"]))
    assert control[1, 1, 2] == level(p1) and control[1, 1, 7] == level(p1 - np.float32(P["drop"]))
    assert control[3, 1, 16 + 16 + 4] == level(P["silence"]) and control[2, 1, 16 + 5 + 4] == level(P["silence"])
    assert np.all(f0[1, :7] == np.float32(220.0))                     # no vibrato through its delay: A3 exactly


# ---- (b) chunking ----------------------------------------------------------------------------------------------------------------
def test_a_voices_bits_do_not_depend_on_the_hop_size(runs):
    f0_1, control_1, active_1 = runs[1]
    assert int(active_1.sum()) == 48 + 10 + 21 + 8
    for K in (2, 16):
        f0, control, active = runs[K]
        assert bool((active | ~active_1).all())                       # a longer hop only adds frames behind the release's end
        assert torch.equal(f0[active_1], f0_1[active_1])
        for c in (0, 1):
            assert torch.equal(control[:, c][active_1], control_1[:, c][active_1])


# ---- (c) a held note -------------------------------------------------------------------------------------------------------------
def test_a_note_held_for_40000_frames():
    """2 500 hops of 16 through the op alone: the last hop against the restatement under (a)'s bar (a phase formed in float32 would
    miss it by 4x: test_cpu_note_player.py); slot 1 idle, slot 2 releasing throughout: exactly 0"""
    p = nc.params(attack=3, decay=4, release=5, vib_rate=5.5, vib_depth=40.0)
    state, params = new_state(3), params_tensor(p)
    notes = notes_tensor([(64.3, 0.7, nc.HELD), (50.0, 0.5, nc.HELD), (50.0, 0.5, 0)])
    f0 = torch.full((3, 16), 7.0, device="cuda")
    control = torch.full((3, 2, 16), 7.0, device="cuda")
    first = torch.tensor([nc.ACTIVE | nc.START, 0, nc.RELEASE], dtype=torch.int32).cuda()
    later = torch.tensor([nc.ACTIVE, 0, nc.RELEASE], dtype=torch.int32).cuda()
    for h in range(2500):
        ops().note_control(params, first if h == 0 else later, notes, state, f0, control)
    f0, control = f0.cpu().numpy(), control.cpu().numpy()
    assert int(state[:4].cpu().view(torch.int32)[0]) == 40000
    j = np.arange(40000 - 16, 40000)
    sel = np.ones(16, dtype=bool)
    f0_64, control_64, _ = nc.note(j, 64.3, 0.7, nc.HELD, p)
    f0_32, control_32, _ = nc.note(j, 64.3, 0.7, nc.HELD, p, np.float32)
    d = distances(f0[0], control[0], f0_64, control_64, p, sel)
    yard = distances(f0_32.astype(np.float64), control_32.astype(np.float64), f0_64, control_64, p, sel)
    record("note_control_held_40000", loudness_err=d[0], loudness_yardstick=yard[0], f0_rel_err=d[1], f0_rel_yardstick=yard[1],
           control0_rel_err=d[2])
    print("held note, frames 39984 .. 39999: kernel", d, "yardstick", yard)
    bar = bars(yard)
    assert d[0] <= bar[0] and d[1] <= bar[1] and d[2] <= bar[2], (d, yard, bar)
    assert not f0[1:].any() and not control[1:].any()


# ---- (d) the mix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots, N", [(3, 128), (17, 2048 + 3)])
@pytest.mark.parametrize("C", [1, 2])
def test_voice_mix(n_slots, N, C):
    g = torch.Generator().manual_seed(n_slots * 10 + C)
    o = torch.randn(n_slots, N, generator=g).cuda()
    gain = torch.randn(n_slots, C, generator=g).cuda()
    out = torch.full((C, N), 7.0, device="cuda")
    ops().voice_mix(o, gain, out)
    again = torch.full((C, N), -7.0, device="cuda")
    ops().voice_mix(o, gain, again)
    assert torch.equal(out, again)                                    # no atomics: two calls, equal bits
    want, scale = nc.voice_mix(o.cpu().numpy(), gain.cpu().numpy())
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    record(f"voice_mix_B{n_slots}_N{N}_C{C}", max_err_over_scale=float((err / scale).max()))
    assert np.all(err <= 1e-6 * scale)
    # a zero gain removes its slot exactly: the same bits as the mix without that slot, whatever the slot holds
    b = n_slots // 2
    gain0, o0 = gain.clone(), o.clone()
    gain0[b] = 0.0
    o0[b] = 1e30
    keep = [i for i in range(n_slots) if i != b]
    without = torch.empty((C, N), device="cuda")
    ops().voice_mix(o[keep].contiguous(), gain[keep].contiguous(), without)
    ops().voice_mix(o0, gain0, out)
    assert torch.equal(out, without)
    # rows that are not 16-byte aligned take the scalar kernel: the same bits as the aligned call
    if N % 4 == 0:
        shifted = torch.empty(n_slots * N + 1, device="cuda")[1:].view(n_slots, N).copy_(o)
        ops().voice_mix(shifted, gain, out)
        assert torch.equal(out, again)


# ---- (e) the player end to end -------------------------------------------------------------------------------------------------------
# (on frame, off frame, pitch, velocity, pan): four notes on two slots - a slot is taken again while its reverb tail still rings
SCORE = [(0, 8, 57.0, 0.9, -0.5), (2, 6, 64.0, 0.5, 0.5), (12, 18, 60.0, 0.7, 0.0), (16, 20, 67.0, 1.0, 1.0)]
E_FRAMES = 32
ENVELOPE = dict(attack=1, decay=2, release=3, vib_delay=2, vib_ramp=4, vib_depth=20.0)


@pytest.fixture(scope="module")
def model():
    return build_model(True)


@pytest.fixture(scope="module")
def draws():
    g = torch.Generator().manual_seed(27)
    return torch.rand(101, generator=g).cuda(), torch.rand(128 * E_FRAMES - 1, generator=g).cuda()


def normalisation():
    z = load_npz("weights_vn.npz")
    return z["__data_mean__"].astype(np.float64), z["__data_std__"].astype(np.float64)


def play_by_frames(player, K):
    """SCORE through the player in hops of K frames -> the output, and per hop what the hop fed its stream"""
    out, fed, handles = [], [], {}
    for h in range(E_FRAMES // K):
        for i, (on, off, pitch, velocity, pan) in enumerate(SCORE):
            if on == h * K:
                handles[i] = player.note_on(pitch, velocity, pan)
                assert handles[i] is not None
            if off == h * K:
                player.note_off(handles[i])
        out.append(player.hop().clone())
        f0, control, start, stop, o = player.last_hop
        fed.append((f0.clone(), control.clone(), list(start), list(stop), np.array(player.book.gains, dtype=np.float64)))
    return torch.cat(out, 1), fed


@pytest.fixture(scope="module")
def played(model, draws):
    res = {}
    for K in (1, 2):
        player = model.player(2, hop_frames=K, channels=2, normalisation=normalisation(), phase_u=draws[0], noise=draws[1], **ENVELOPE)
        y, fed = play_by_frames(player, K)
        states = player.stream.slot_states()
        active = player.active()
        player.check()
        player.close()
        res[K] = (y.cpu().numpy(), fed, states, active, player.dropped)
    return res


@pytest.mark.parametrize("K", [1, 2])
def test_player_equals_a_voice_stream_driven_by_hand(model, draws, played, K):
    y, fed, states, active, dropped = played[K]
    assert y.shape == (2, 128 * E_FRAMES) and np.isfinite(y).all()
    assert states == ["idle", "idle"] and active == [] and dropped == 0
    starts = [s for f in fed for s in f[2]]
    assert sorted(starts) == [0, 0, 1, 1]                              # both slots used twice
    ref = model.stream(2, slots=True, phase_u=draws[0], noise=draws[1])
    want = []
    for f0, control, start, stop, gains in fed:
        o = ref.push(f0.unsqueeze(1), control, start=start, stop=stop).cpu().numpy().astype(np.float64)
        want.append(gains.T @ o)
    ref.close()
    want = np.concatenate(want, 1)
    err, level = rms(y - want), rms(want)
    record(f"note_player_K{K}", y_rms_err=err, y_rms=level)
    print(f"player K {K}: rms {level:.3e}, rms err {err:.3e}")
    assert level > 0 and want[0].any() and want[1].any()
    assert err <= 1e-6
    # what the player fed is the restatement's note: the last note starts at frame 16 and is released from its frame 4 on
    mean, std = normalisation()
    p = nc.params(**ENVELOPE, vib_rate=5.5, drop=0.075, peak_hi=min(1.0, mean[1] + 2 * std[1]), peak_lo=mean[1] - std[1],
                  silence=max(0.0, mean[1] - 4 * std[1]), mean0=mean[0], std0=std[0], mean1=mean[1], std1=std[1])
    b = fed[16 // K][2][0]
    f0_fed = torch.cat([f[0] for f in fed], 1).cpu().numpy()[b, 16:22]
    l_fed = torch.cat([f[1] for f in fed], 2).cpu().numpy()[b, 1, 16:22] * std[1] + mean[1]
    f0_64, _, l_64 = nc.note(np.arange(6), 67.0, 1.0, 4, p)
    assert np.abs(f0_fed / f0_64 - 1).max() <= FLOOR_F0 and np.abs(l_fed - l_64).max() <= FLOOR_L


# ---- (f) the script ------------------------------------------------------------------------------------------------------------------
def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_play_score_script(model, draws, played, tmp_path):
    ps = _script("play_score")
    csv = tmp_path / "score.csv"
    rows = ["# onset_s,duration_s,pitch,velocity,pan", ""]
    rows += [f"{on * 128 / 16000!r}, {(off - on) * 128 / 16000!r}, {pitch}, {velocity}, {pan}  # note" for on, off, pitch, velocity, pan in SCORE]
    csv.write_text("\n".join(rows) + "\n")
    notes = ps.read_score(str(csv))
    assert len(notes) == 4 and notes[1][2:] == (64.0, 0.5, 0.5)
    assert ps.hop_events(notes, 128, 16000) == {0: ([0], []), 2: ([1], []), 6: ([], [1]), 8: ([], [0]), 12: ([2], []), 18: ([], [2]),
                                                  16: ([3], []), 20: ([], [3])}
    player = model.player(2, hop_frames=1, channels=2, normalisation=normalisation(), phase_u=draws[0], noise=draws[1], **ENVELOPE)
    y, dropped = ps.play(player, notes, 16000, 8 * 128 / 16000)
    player.close()
    # the last note's release ends in hop 22, its slot is idle after hop 23; 8 hops of tail
    assert dropped == 0 and y.shape == (2, 128 * (24 + 8))
    assert np.array_equal(y, played[1][0])                             # the same score and draws as (e): the same bits
    # and the command itself: a mono file of the expected length
    from click.testing import CliRunner
    from scipy.io import wavfile
    wav = tmp_path / "out.wav"
    r = CliRunner().invoke(ps.main, [str(csv), str(wav), "--use-fastnewt", "--voices", "2", "--hop-frames", "2", "--tail-seconds", "0.032",
                                     "--release", "3", "--seed", "1"])
    assert r.exit_code == 0, r.output
    sr, x = wavfile.read(str(wav))
    # K = 2: the last note (on 16, off 20, release 3) stops in hop 11 (frames 22, 23), idle after hop 12; 2 hops of tail
    assert sr == 16000 and x.dtype == np.float32 and x.shape == (256 * (13 + 2),) and np.isfinite(x).all() and x.any()


# ---- (g) refusals on the device ---------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_leave_the_outputs_alone(runs):
    K = 16
    state, params = new_state(B), params_tensor(P)
    hops = schedule(K)
    f0 = torch.full((B, K), 7.0, device="cuda")
    control = torch.full((B, 2, K), 7.0, device="cuda")
    ev, notes = torch.tensor(hops[0][0], dtype=torch.int32).cuda(), notes_tensor(hops[0][1])
    bad = dict(P, release=0)
    calls = [lambda: ops().note_control(params_tensor(bad), ev, notes, state, f0, control),
             lambda: ops().note_control(params_tensor(dict(P, vib_ramp=0)), ev, notes, state, f0, control),
             lambda: ops().note_control(params[:15].clone(), ev, notes, state, f0, control),
             lambda: ops().note_control(params, ev[:4].contiguous(), notes, state, f0, control),
             lambda: ops().note_control(params, ev, notes[:, :3].contiguous(), state, f0, control),
             lambda: ops().note_control(params, ev, notes, state[:8], f0, control),
             lambda: ops().note_control(params, ev, notes, state, f0, control[:, :1].contiguous()),
             lambda: ops().note_control(params, ev, notes, state, torch.full((B, 17), 7.0, device="cuda"), torch.full((B, 2, 17), 7.0, device="cuda")),
             lambda: ops().note_control(params, ev.cpu(), notes, state, f0, control),
             lambda: ops().note_control_reset(state[:8], B),
             lambda: ops().note_control_reset(state, 65536)]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"call {i} was accepted")
    # the C entry points themselves, on device pointers
    L = lib()
    struct = importlib.import_module(PKG + "._cops").CtypesOps._note_player
    import ctypes as C
    ok = struct(params)
    args = (ev.data_ptr(), notes.data_ptr(), state.data_ptr(), state.numel())
    assert L.nws_note_control(C.byref(ok), *args, B, 17, f0.data_ptr(), control.data_ptr(), None) == -2
    assert L.nws_note_control(C.byref(ok), *args, 65536, K, f0.data_ptr(), control.data_ptr(), None) == -1
    assert L.nws_note_control(C.byref(struct(params_tensor(bad))), *args, B, K, f0.data_ptr(), control.data_ptr(), None) == -2
    assert L.nws_note_control(C.byref(ok), args[0], args[1], args[2], 4 * B - 1, B, K, f0.data_ptr(), control.data_ptr(), None) == -2
    o, gain, out = torch.ones(3, 128, device="cuda"), torch.ones(3, 3, device="cuda"), torch.full((3, 128), 7.0, device="cuda")
    with pytest.raises(RuntimeError):
        ops().voice_mix(o, gain, out)
    with pytest.raises(RuntimeError):
        ops().voice_mix(o, gain[:, :2].contiguous(), out)             # out (3, N) for two channels
    assert L.nws_voice_mix(o.data_ptr(), gain.data_ptr(), 3, 128, 3, out.data_ptr(), None) == -2
    assert L.nws_voice_mix(o.data_ptr(), gain.data_ptr(), 65536, 128, 1, out.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((f0 == 7.0).all()) and bool((control == 7.0).all()) and bool((out == 7.0).all())
    assert not state.cpu().any()                                      # and the counters are still those of the reset
    # a valid call afterwards: (a)'s bits
    got_f0, got_control, _ = run_kernel(K)
    assert torch.equal(got_f0, runs[K][0]) and torch.equal(got_control, runs[K][1])
    ops().note_control(params, ev, notes, state, f0, control)       # and on the buffers the refusals left alone
    assert torch.equal(f0.cpu(), runs[K][0][:, :K]) and torch.equal(control.cpu(), runs[K][1][:, :, :K])


# ---- (h) the other binding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("NWS_BACKEND") == "ctypes", reason="already the ctypes pass")
def test_note_player_through_the_ctypes_binding():
    """every test of this file again through the torch-free ctypes binding"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_note_player.py"), "-k", "not through_the"],
                       env=dict(os.environ, NWS_BACKEND="ctypes"), capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
