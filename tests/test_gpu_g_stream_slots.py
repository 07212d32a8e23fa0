"""-m gpu: slot mode on the runtime-size stream (csrc/generic.hip nws_g_stream_step_slots) - `model.voices(B)` and
`model.player(voices)` on a model `Engine.specialised()` turns down.  Anchor, as for the packaged slot stream
(tests/test_gpu_stream_slots.py, whose schedule, events, poisoning and one-frame oracle are used here): every voice is the
oracle's ONE-SHOT `pre_reverb` of its own (f0, control) with the stream's phase draw and its own slice of the stream's noise,
placed at 128 a_v + 64 of its slot's output; the slot's output is its dry signal plus a float64 linear convolution with [0, ir].
Sizes: tests/g_stream_models.py - `bank` as FastNEWT, `odd` with exact shapers - and the packaged model."""
import copy
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.signal import fftconvolve

from conftest import ROOT, load_npz, rms
from g_stream_models import SIZES, build, oracle_for
from gpu_util import build_model, maxabs, record
from test_gpu_stream_slots import events, one_frame_oracle, run, schedule

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED, WORKSPACE = -2, -1, -3     # include/nws_hip.h
PKG = "neural-waveshaping-synthesis_amd"


def streaming():
    return importlib.import_module(PKG + ".streaming")


@pytest.fixture(scope="module")
def models():
    """sizes -> (model, oracle, impulse response): built once, shared, never edited (tests that edit weights build their own)"""
    cache = {}

    def get(sizes):
        if sizes not in cache:
            fast = sizes == "bank"
            model, w = build(sizes, fast)
            assert not model._engine.specialised()
            cache[sizes] = (model, oracle_for(sizes, w, fast), w["reverb.ir"].reshape(-1).astype(np.float64))
        return cache[sizes]

    return get


def inputs(n_harmonics, B, F, seed, voices, K):
    """tests/test_gpu_stream_slots.py's inputs with the model's harmonic count: NaN / inf in every frame no voice covers"""
    g = torch.Generator().manual_seed(seed)
    f0 = (120 + 600 * torch.rand(B, 1, 1, generator=g)) * (1 + 0.03 * torch.randn(B, 1, F, generator=g))
    control = torch.randn(B, 2, F, generator=g)
    live = torch.zeros(B, F, dtype=torch.bool)
    for b, vs in voices.items():
        for s, n in vs:
            live[b, s * K:(s + n) * K] = True
    f0[:, 0][~live] = float("nan")
    control[:, 1][~live] = float("inf")
    pu, nz = torch.rand(n_harmonics, generator=g), torch.rand(128 * F - 1, generator=g)
    return f0, control, pu, nz


def expected(model, oracle, ir, voices, f0, control, pu, nz, K, F):
    """-> (dry, y_ref, yardstick): the placed one-shot voices, their float64 reverb, and the largest distance of the MODEL's own
    one-shot pre_reverb from the oracle's on a voice's inputs (voices of at least two frames: the one-shot refuses one)"""
    B = f0.shape[0]
    dry = np.zeros((B, 128 * F), np.float64)
    yard = 0.0
    for b, vs in voices.items():
        for s, n in vs:
            a, T = s * K, n * K
            st = {}
            fv, cv, zv = f0[b:b + 1, :, a:a + T], control[b:b + 1, :, a:a + T], nz[128 * a:128 * (a + T) - 1]
            (one_frame_oracle(oracle) if T == 1 else oracle)(fv, cv, pu, zv, stages=st)
            want = st["pre_reverb"].numpy()[0]
            dry[b, 128 * a + 64:128 * (a + T) + 64] += want
            if T >= 2:
                with torch.no_grad():
                    own = model.pre_reverb(fv.cuda(), cv.cuda(), phase_u=pu.cuda(), noise=zv.contiguous().cuda()).cpu().numpy().reshape(-1)
                yard = max(yard, maxabs(own, want))
    ir_ = np.concatenate([[0.0], ir])
    wet = np.stack([fftconvolve(dry[b], ir_)[:128 * F] for b in range(B)])
    return dry, dry + wet, yard


def pre_bar(dry, yard):
    """2e-6 * max(1, max|dry| / 1e-2); where 4 x the model's own one-shot distance from the oracle exceeds it, that"""
    bar = 2e-6 * max(1.0, float(np.abs(dry).max()) / 1e-2)
    return (4.0 * yard, True) if 4.0 * yard > bar else (bar, False)


def judge(name, y, pre, dry, y_ref, voices, yard):
    e_pre, e_y = maxabs(pre, dry), rms(y - y_ref)
    bar, invoked = pre_bar(dry, yard)
    print(name, dict(e_pre=e_pre, bar=bar, yardstick=yard, exception_invoked=invoked, pre_max=float(np.abs(dry).max()), e_y=e_y,
                     y_rms=rms(y_ref)))
    record(name, pre_max_abs_err=e_pre, pre_bar=bar, one_shot_pre_max_abs_err=yard, bar_exception_invoked=invoked,
           pre_max=float(np.abs(dry).max()), y_rms_err=e_y, y_rms=rms(y_ref))
    assert np.isfinite(y).all() and np.isfinite(pre).all()
    assert e_pre <= bar
    assert e_y <= 1e-4 * max(1.0, rms(y_ref))
    for b, vs in voices.items():
        if not vs:
            assert not y[b].any() and not pre[b].any(), f"never-used slot {b} is not exactly 0"


# ---- (a) schedule parity against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,B,K", [("bank", 3, 1), ("bank", 3, 2), ("odd", 3, 1), ("odd", 3, 2), ("bank", 3, 16), ("bank", 17, 2)])
def test_slot_schedule_parity(models, sizes, B, K):
    model, oracle, ir = models(sizes)
    H = 9
    F = H * K
    voices = schedule(B, H)
    start, stop = events(voices, B, H)
    f0, control, pu, nz = inputs(SIZES[sizes][3], B, F, 100 * B + K, voices, K)
    s = model.voices(B, phase_u=pu.cuda(), noise=nz.cuda())
    assert type(s) is streaming().GenericVoiceStream
    y, pre = run(s, f0, control, K, H, start, stop)
    assert y.shape == (B, 128 * F) and s.idle_slots() == [b for b in range(B)]
    dry, y_ref, yard = expected(model, oracle, ir, voices, f0, control, pu, nz, K, F)
    judge(f"g_slots_{sizes}_B{B}_K{K}", y, pre, dry, y_ref, voices, yard)
    s.check()
    s.close()


# ---- (b) a voice does not know it is in a slot -----------------------------------------------------------------------------------
def test_a_voice_is_the_plain_stream_of_its_own_frames(models):
    """Slot 1 of three gets one voice of three hops at hop 2; a GenericNewtStream(B = 1) is pushed the same frames in the same
    chunks with the voice's noise slice and final=True.  The bar is (a)'s; the distance itself is recorded (measured: 0.0 - see
    DESIGN.md 3.28 for why the duplicated first frame reproduces the one-shot's left clamp to the bit)."""
    model, oracle, ir = models("bank")
    B, K, H = 3, 2, 7
    voices = {0: [], 1: [(2, 3)], 2: []}
    start, stop = events(voices, B, H)
    f0, control, pu, nz = inputs(SIZES["bank"][3], B, H * K, 41, voices, K)
    s = model.voices(B, phase_u=pu.cuda(), noise=nz.cuda())
    y, pre = run(s, f0, control, K, H, start, stop)
    s.close()
    a, T = 2 * K, 3 * K
    seg = pre[1, 128 * a + 64:128 * (a + T) + 64]
    p = model.stream(1, phase_u=pu.cuda(), noise=nz[128 * a:128 * (a + T) - 1].contiguous().cuda())
    assert type(p) is streaming().GenericNewtStream
    ps = []
    for h in range(3):
        k0 = a + h * K
        p.push(f0[1:2, :, k0:k0 + K].cuda(), control[1:2, :, k0:k0 + K].cuda(), final=h == 2)
        ps.append(p._last_pre.cpu().numpy())
    alone = np.concatenate(ps, 1)[0]
    assert alone.shape == seg.shape == (128 * T,)
    dry, y_ref, yard = expected(model, oracle, ir, voices, f0, control, pu, nz, K, H * K)
    bar, _ = pre_bar(dry, yard)
    dist = maxabs(seg, alone)
    print("voice in a slot against the plain stream of its frames: max-abs", dist, "bit-identical", bool(np.array_equal(seg, alone)), "bar", bar)
    record("g_slots_voice_vs_plain_stream", pre_max_abs_distance=dist, bit_identical=bool(np.array_equal(seg, alone)), pre_bar=bar)
    assert dist <= bar
    assert not pre[1, :128 * a + 64].any() and not pre[1, 128 * (a + T) + 64:].any() and not pre[0].any() and not pre[2].any()
    judge("g_slots_single_voice", y, pre, dry, y_ref, voices, yard)


# ---- (c) runtime-size against packaged ----------------------------------------------------------------------------------------
def test_runtime_size_slots_on_the_packaged_model(weights):
    from oracle.newt_oracle import OracleNEWT

    model = build_model(True)
    oracle = OracleNEWT(weights, fast=True, lut_python_loop=False)
    ir = weights["reverb.ir"][0].astype(np.float64)
    B, K, H = 3, 2, 9
    F = H * K
    voices = schedule(B, H)
    start, stop = events(voices, B, H)
    f0, control, pu, nz = inputs(101, B, F, 100 * B + K, voices, K)
    dry, y_ref, yard = expected(model, oracle, ir, voices, f0, control, pu, nz, K, F)
    g = streaming().GenericVoiceStream(model, B, phase_u=pu.cuda(), noise=nz.cuda())
    yg, pg = run(g, f0, control, K, H, start, stop)
    g.close()
    v = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda())
    assert type(v) is streaming().VoiceStream
    yv, pv = run(v, f0, control, K, H, start, stop)
    v.close()
    judge("g_slots_packaged_runtime_size", yg, pg, dry, y_ref, voices, yard)
    judge("g_slots_packaged_fused", yv, pv, dry, y_ref, voices, yard)
    d_pre, d_y = maxabs(pg, pv), rms(yg - yv)
    print("runtime-size against fused slot stream on the packaged model: pre max-abs", d_pre, "y rms", d_y, "of", rms(yv))
    record("g_slots_packaged_runtime_size_vs_fused", pre_max_abs_distance=d_pre, y_rms_distance=d_y, y_rms=rms(yv))


# ---- (d) chunking ------------------------------------------------------------------------------------------------------------------
def test_hop_size_changes_no_bit_of_the_dry_signal(models):
    """16 frames as sixteen one-frame hops and as eight two-frame hops (events on even frames): `pre` bit for bit, the output to 1e-5
    of its RMS (the reverb sums its taps per hop, so its order differs)."""
    model, _, _ = models("bank")
    B, F = 3, 16
    frames = {0: [(0, 6), (8, 2)], 1: [(4, 8)], 2: []}                # (first frame, frames) per voice
    f0, control, pu, nz = inputs(SIZES["bank"][3], B, F, 77, frames, 1)
    got = {}
    for K in (1, 2):
        voices = {b: [(a // K, n // K) for a, n in vs] for b, vs in frames.items()}
        start, stop = events(voices, B, F // K)
        s = model.voices(B, phase_u=pu.cuda(), noise=nz.cuda())
        got[K] = run(s, f0, control, K, F // K, start, stop)
        s.close()
    (y1, p1), (y2, p2) = got[1], got[2]
    assert np.isfinite(y1).all() and p1[0].any() and p1[1].any() and not p1[2].any()
    print("K = 1 against K = 2: pre max-abs", maxabs(p1, p2), "y rms", rms(y1 - y2), "of", rms(y1))
    record("g_slots_chunking_K1_vs_K2", pre_max_abs_distance=maxabs(p1, p2), y_rms_distance=rms(y1 - y2), y_rms=rms(y1))
    assert np.array_equal(p1, p2)
    assert rms(y1 - y2) <= 1e-5 * rms(y1)


# ---- (e) graph and eager -------------------------------------------------------------------------------------------------------------
def test_captured_hop_equals_eager_also_after_a_weight_edit():
    model, _ = build("bank", False)
    B, K, H = 3, 2, 9
    voices = schedule(B, H)
    more = {0: [(0, 2)], 1: [(1, 1)], 2: []}                           # four more hops after the edit
    start, stop = events(voices, B, H)
    start2, stop2 = events(more, B, 4)
    f0, control, pu, nz = inputs(SIZES["bank"][3], B, (H + 4) * K, 9, {b: voices[b] + [(H + s, n) for s, n in more[b]] for b in voices}, K)
    a = model.voices(B, phase_u=pu.cuda(), noise=nz.cuda(), graph=False)
    b = model.voices(B, phase_u=pu.cuda(), noise=nz.cuda())
    ya, pa = run(a, f0, control, K, H, start, stop)
    yb, pb = run(b, f0, control, K, H, start, stop, static=True)
    assert len(a._graphs) == 0 and len(b._graphs) == 1                 # one captured hop while the events change hop by hop
    assert ya.any() and np.array_equal(ya, yb) and np.array_equal(pa, pb)
    with torch.no_grad():
        model.newt.mixer[0].bias.add_(0.05)                            # in place: nobody tells the engine
    a.refresh()
    b.refresh()
    assert not b._graphs                                               # dropped: it pointed into the old descriptor's tables
    f2, c2 = f0[:, :, H * K:], control[:, :, H * K:]
    ya2, pa2 = run(a, f2, c2, K, 4, start2, stop2)
    yb2, pb2 = run(b, f2, c2, K, 4, start2, stop2, static=True)
    assert len(b._graphs) == 1
    assert ya2.any() and np.array_equal(ya2, yb2) and np.array_equal(pa2, pb2)
    a.close()
    b.close()


# ---- (f) the player ------------------------------------------------------------------------------------------------------------------
def test_player_on_the_bank_equals_a_slot_stream_driven_by_hand(models):
    model, _, _ = models("bank")
    z = load_npz("weights_vn.npz")
    norm = (z["__data_mean__"].astype(np.float64), z["__data_std__"].astype(np.float64))
    K, hops = 2, 8
    g = torch.Generator().manual_seed(28)
    pu, nz = torch.rand(SIZES["bank"][3], generator=g).cuda(), torch.rand(128 * K * hops - 1, generator=g).cuda()
    player = model.player(2, hop_frames=K, channels=2, normalisation=norm, phase_u=pu, noise=nz, attack=1, decay=4, release=3,
                          vib_delay=2, vib_ramp=4, vib_depth=20.0)
    assert type(player.stream) is streaming().GenericVoiceStream
    out, fed = [], []
    for h in range(hops):
        if h == 0:
            held = player.note_on(57.0, 0.9, -0.5)                     # held to the end
            short = player.note_on(64.0, 0.5, 0.5)
            assert held is not None and short is not None
            assert player.note_on(60.0, 0.7, 0.0) is None              # no slot: dropped, nobody is stolen from
        if h == 1:
            player.note_off(short)                                     # from its frame 2 on: inside the decay (frames 1 .. 4)
        out.append(player.hop().clone())
        f0, control, start, stop, o = player.last_hop
        fed.append((f0.clone(), control.clone(), list(start), list(stop), np.array(player.book.gains, dtype=np.float64)))
    y = torch.cat(out, 1).cpu().numpy()
    assert player.dropped == 1 and player.active() == [held]
    assert player.stream.slot_states() == ["active", "idle"]
    assert [f[3] for f in fed][2] == [1]                               # j_off + R - 1 = 4: the slot's stop rides on hop 2
    player.check()
    player.close()
    ref = streaming().GenericVoiceStream(model, 2, phase_u=pu, noise=nz)
    want = []
    for f0, control, start, stop, gains in fed:
        o = ref.push(f0.unsqueeze(1), control, start=start, stop=stop).cpu().numpy().astype(np.float64)
        want.append(gains.T @ o)
    ref.close()
    want = np.concatenate(want, 1)
    err, level = rms(y - want), rms(want)
    print(f"player on the bank: rms {level:.3e}, rms err {err:.3e}")
    record("g_slots_note_player_bank_K2", y_rms_err=err, y_rms=level)
    assert y.shape == (2, 128 * K * hops) and np.isfinite(y).all() and level > 0 and want[0].any() and want[1].any()
    assert err <= 1e-6 * level


# ---- (g) refusals on the device --------------------------------------------------------------------------------------------------------
def test_refused_calls_touch_nothing(models):
    """Raw C ABI on device buffers: refused calls return their codes before anything is launched - out still NaN, the state still
    its fill pattern - and a valid call right after gives the op's bits."""
    _lib = importlib.import_module(PKG + "._lib")
    engine = importlib.import_module(PKG + ".engine")
    model, _, _ = models("bank")
    L = _lib.lib()
    r = model._engine.generic.model_desc()
    g, dev = r.struct, r.device
    B, K, maxf = 2, 2, 4
    nbytes = L.nws_g_stream_slot_state_bytes(C.byref(g), B, maxf, g.ir_len)
    assert nbytes >= L.nws_g_stream_state_bytes(C.byref(g), B, maxf, g.ir_len, None) > 0
    gen = torch.Generator().manual_seed(1)
    f0d = (200 + 100 * torch.rand(B, K, generator=gen)).cuda()
    cd, pud, nzd = torch.randn(B, 2, K, generator=gen).cuda(), torch.rand(g.n_harmonics, generator=gen).cuda(), torch.rand(128 * 8).cuda()
    ev = torch.zeros(B, dtype=torch.int32, device=dev)
    M = L.nws_stream_out_samples(K, 1, 0)
    out = torch.full((B, M), float("nan"), device=dev)
    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    st = engine.stream_ptr(dev)

    def call(state_ptr=None, nb=nbytes, f0p=None, outp=None, evp=None, k=K, mf=maxf):
        return L.nws_g_stream_step_slots(C.byref(g), state.data_ptr() if state_ptr is None else state_ptr, nb, B, mf,
                                         f0d.data_ptr() if f0p is None else f0p, cd.data_ptr(), 2, k, 0, 0, float(model.osc.sample_rate),
                                         pud.data_ptr(), r.rand_phase.data_ptr(), None, nzd.data_ptr(), nzd.numel(),
                                         ev.data_ptr() if evp is None else evp, out.data_ptr() if outp is None else outp, None, st)

    null = C.c_void_p(None)
    assert call(evp=null) == BAD_ARG
    assert call(state_ptr=null) == BAD_ARG and call(f0p=null) == BAD_ARG and call(outp=null) == BAD_ARG
    assert call(k=0) == BAD_ARG and call(k=maxf + 1) == BAD_ARG
    assert call(k=17, mf=17) == UNSUPPORTED and call(mf=17) == UNSUPPORTED
    assert call(nb=nbytes - 4) == WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((state == 0x5A).all())
    _lib.check(L.nws_stream_reset(state.data_ptr(), nbytes, st), "nws_stream_reset")
    assert call() == 0
    state2 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    out2 = torch.empty_like(out)
    engine.binding().g_stream_step_slots(r.gdesc, state2, maxf, f0d, cd, 0, 0, float(model.osc.sample_rate), pud, r.rand_phase, None, nzd,
                                         ev, out2, None)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, out2)
    assert not out.any()                                               # the pre-roll: every row idle


# ---- (h) the ctypes binding ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("NWS_BACKEND") == "ctypes", reason="already the ctypes pass")
def test_g_slots_through_the_ctypes_binding():
    """every test of this file again through the torch-free ctypes binding of nws_g_stream_step_slots, in a fresh process"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_g_stream_slots.py"), "-k", "not through_the"],
                       env=dict(os.environ, NWS_BACKEND="ctypes"), capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
