"""-m gpu tests of the slot mode of the stateful stream (`model.stream(B, slots=True)`, streaming.VoiceStream): B voices that
start and stop on their own in one batched stream.  Anchor: every voice is the oracle's ONE-SHOT `pre_reverb` of its own
(f0, control), with the stream's phase draw and its own slice of the stream's noise, placed at 128 a_v + 64 of its slot's
output; the slot's output is its dry signal plus the linear reverb of it (a float64 convolution)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.signal import fftconvolve

from conftest import ROOT, rms
from gpu_util import build_model, maxabs, record
from stream_long import reverb_errors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(weights):
    from oracle.newt_oracle import OracleNEWT

    return build_model(True), OracleNEWT(weights, fast=True, lut_python_loop=False), weights


def schedule(B, H):
    """voices per slot as (start hop, hops).  Slot 0: a voice from hop 0, restarted after its release while the first voice's
    reverb tail still rings, then a voice that starts and stops in one hop, then another; slot 1 starts later; slot 2 and every
    fourth slot from 3 on stay idle throughout (fed NaN)."""
    v = {0: [(0, 3), (4, 1), (6, 2)], 1: [(2, 4)], 2: []}
    for b in range(3, B):
        v[b] = [] if b % 4 == 3 else [(b % 5, 1 + b % 3)]
    assert all(s + n < H for vs in v.values() for s, n in vs)          # every release hop inside the run
    return v


def events(voices, B, H):
    start = [[] for _ in range(H)]
    stop = [[] for _ in range(H)]
    for b, vs in voices.items():
        for s, n in vs:
            start[s].append(b)
            stop[s + n - 1].append(b)
    return start, stop


def inputs(B, F, seed, voices, K):
    g = torch.Generator().manual_seed(seed)
    f0 = (120 + 600 * torch.rand(B, 1, 1, generator=g)) * (1 + 0.03 * torch.randn(B, 1, F, generator=g))
    control = torch.randn(B, 2, F, generator=g)
    # idle / releasing frames of a slot are never read into an output: poison them
    live = torch.zeros(B, F, dtype=torch.bool)
    for b, vs in voices.items():
        for s, n in vs:
            live[b, s * K:(s + n) * K] = True
    f0[:, 0][~live] = float("nan")
    control[:, 1][~live] = float("inf")
    pu, nz = torch.rand(101, generator=g), torch.rand(128 * F - 1, generator=g)
    return f0, control, pu, nz


def one_frame_oracle(oracle):
    """The reference's torch.stft(center=True) refuses to reflect-pad 128 samples on both sides of a one-frame voice's 127 noise
    samples; the stream reflects again at the other end (what numpy's reflect padding does).  Same oracle otherwise."""
    import types

    def fir_noise(self, H_re, noise):
        hop = self.control_hop
        padded = torch.from_numpy(np.pad(noise.numpy(), self.ir_length // 2, mode="reflect"))
        H_z = torch.complex(H_re, torch.zeros_like(H_re))
        h = torch.fft.irfft(H_z.transpose(1, 2)).roll(self.ir_length // 2, -1) * self.window.view(1, 1, -1)
        X = torch.stft(padded, self.ir_length, hop, center=False, return_complex=True).unsqueeze(0)
        y = torch.istft(X * torch.fft.rfft(h).transpose(1, 2), self.ir_length, hop, center=False)
        return y.unsqueeze(1)[:, :, : H_re.shape[-1] * hop]

    oracle_1 = type(oracle).__new__(type(oracle))
    oracle_1.__dict__.update(oracle.__dict__)
    oracle_1.fir_noise = types.MethodType(fir_noise, oracle_1)
    return oracle_1


def expected(oracle, weights, voices, f0, control, pu, nz, K, F):
    B = f0.shape[0]
    dry = np.zeros((B, 128 * F), np.float64)
    for b, vs in voices.items():
        for s, n in vs:
            a, T = s * K, n * K
            st = {}
            (one_frame_oracle(oracle) if T == 1 else oracle)(f0[b:b + 1, :, a:a + T], control[b:b + 1, :, a:a + T], pu,
                                                             nz[128 * a:128 * (a + T) - 1], stages=st)
            dry[b, 128 * a + 64:128 * (a + T) + 64] += st["pre_reverb"].numpy()[0]
    ir_ = np.concatenate([[0.0], weights["reverb.ir"][0].astype(np.float64)])
    wet = np.stack([fftconvolve(dry[b], ir_)[:128 * F] for b in range(B)])
    return dry, dry + wet


def run(s, f0, control, K, H, start, stop, static=False):
    ys, pres = [], []
    for h in range(H):
        f, c = f0[:, :, h * K:(h + 1) * K].cuda(), control[:, :, h * K:(h + 1) * K].cuda()
        if static and h >= 1:
            f0_in, c_in, ev, out = s.static_io(K)
            f0_in.copy_(f[:, 0])
            c_in.copy_(c)
            y = s.hop(K, start=start[h], stop=stop[h]).clone()
        else:
            y = s.push(f, c, start=start[h], stop=stop[h])
        ys.append(y.cpu().numpy())
        pres.append(s._last_pre.cpu().numpy())
    return np.concatenate(ys, 1), np.concatenate(pres, 1)


def judge(name, y, pre, dry, y_ref, voices):
    e_pre = maxabs(pre, dry)
    e_y = rms(y - y_ref)
    record(name, pre_max_abs_err=e_pre, pre_max=float(np.abs(dry).max()), y_rms_err=e_y, y_rms=rms(y_ref))
    assert np.isfinite(y).all() and np.isfinite(pre).all()
    assert e_pre <= 2e-6 * max(1.0, float(np.abs(dry).max()) / 1e-2)
    assert e_y <= 1e-4
    for b, vs in voices.items():
        if not vs:
            assert not y[b].any() and not pre[b].any(), f"never-used slot {b} is not exactly 0"


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("K", [1, 2, 8])
def test_slot_schedule_parity(setup, B, K):
    model, oracle, weights = setup
    H = 9
    F = H * K
    voices = schedule(B, H)
    start, stop = events(voices, B, H)
    f0, control, pu, nz = inputs(B, F, 100 * B + K, voices, K)
    s = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda())
    y, pre = run(s, f0, control, K, H, start, stop)
    assert y.shape == (B, 128 * F)
    dry, y_ref = expected(oracle, weights, voices, f0, control, pu, nz, K, F)
    judge(f"slots_B{B}_K{K}", y, pre, dry, y_ref, voices)
    s.close()


@pytest.mark.parametrize("K", [2, 8])
def test_slot_graph_replay_bit_identical(setup, K):
    """the same schedule eagerly and through static_io / hop: bit for bit, and one captured hop per K while events change"""
    model, _, _ = setup
    B, H = 5, 9
    voices = schedule(B, H)
    start, stop = events(voices, B, H)
    f0, control, pu, nz = inputs(B, H * K, 7 + K, voices, K)
    a = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda(), graph=False)
    ya, pa = run(a, f0, control, K, H, start, stop)
    b = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda())
    yb, pb = run(b, f0, control, K, H, start, stop, static=True)
    assert len(b._graphs) == 1
    assert np.array_equal(ya, yb) and np.array_equal(pa, pb)
    # drawn noise: pushes capture the same single hop
    c = model.stream(B, slots=True, phase_u=pu.cuda())
    for h in range(H):
        y = c.push(f0[:, :, h * K:(h + 1) * K].cuda(), control[:, :, h * K:(h + 1) * K].cuda(), start=start[h], stop=stop[h])
        assert torch.isfinite(y).all()
    assert len(c._graphs) == 1
    c.close()


def test_slot_lockstep_equals_plain_stream(setup):
    """every slot starts at hop 0 and stops at the same hop: a plain NewtStream over the same frames, 64 samples later"""
    model, _, _ = setup
    B, K, H = 3, 2, 6
    F = (H - 1) * K                    # the last hop is the release hop
    g = torch.Generator().manual_seed(5)
    f0 = (120 + 600 * torch.rand(B, 1, 1, generator=g)) * (1 + 0.03 * torch.randn(B, 1, H * K, generator=g))
    control = torch.randn(B, 2, H * K, generator=g)
    pu, nz = torch.rand(101, generator=g), torch.rand(128 * H * K - 1, generator=g)
    s = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda())
    start = [list(range(B))] + [[]] * (H - 1)
    stop = [[]] * (H - 2) + [list(range(B))] + [[]]
    y, pre = run(s, f0, control, K, H, start, stop)
    p = model.stream(B, phase_u=pu.cuda(), noise=nz[:128 * F - 1].cuda())
    ys, ps = [], []
    for h in range(H - 1):
        ys.append(p.push(f0[:, :, h * K:(h + 1) * K].cuda(), control[:, :, h * K:(h + 1) * K].cuda(), final=h == H - 2).cpu().numpy())
        ps.append(p._last_pre.cpu().numpy())
    yp, pp = np.concatenate(ys, 1), np.concatenate(ps, 1)
    assert yp.shape == (B, 128 * F)
    e_pre, e_y = maxabs(pre[:, 64:64 + 128 * F], pp), rms(y[:, 64:64 + 128 * F] - yp)
    record("slots_lockstep_vs_plain", pre_max_abs_err=e_pre, y_rms_err=e_y,
           pre_bit_identical=bool(np.array_equal(pre[:, 64:64 + 128 * F], pp)),
           y_bit_identical=bool(np.array_equal(y[:, 64:64 + 128 * F], yp)))
    assert not pre[:, :64].any() and not pre[:, 64 + 128 * F:].any()
    # same kernels on the same windows: the slot stream IS the plain stream, 64 samples later
    assert np.array_equal(pre[:, 64:64 + 128 * F], pp) and np.array_equal(y[:, 64:64 + 128 * F], yp), (e_pre, e_y)


def test_slot_misuse_raises_and_stream_stays_correct(setup):
    model, oracle, weights = setup
    B, K, H = 3, 2, 9
    F = H * K
    voices = schedule(B, H)
    start, stop = events(voices, B, H)
    f0, control, pu, nz = inputs(B, F, 11, voices, K)
    s = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda())
    ys, pres = [], []
    for h in range(H):
        f, c = f0[:, :, h * K:(h + 1) * K].cuda(), control[:, :, h * K:(h + 1) * K].cuda()
        states = s.slot_states()
        if h == 1:
            with pytest.raises(RuntimeError):
                s.push(f, c, start=[0])                    # start on an active slot
            with pytest.raises(RuntimeError):
                s.push(f, c, stop=[2])                     # stop on an idle slot
            with pytest.raises(RuntimeError):
                s.push(f0[:, :, :17].cuda(), control[:, :, :17].cuda())     # K > 16
            with pytest.raises(RuntimeError):
                s.push(f[:2], c[:2])                       # wrong batch
            with pytest.raises(RuntimeError):
                s.push(f, c[:, :, :1])                     # wrong frame count
        if h == 3:
            assert states[0] == "releasing"
            with pytest.raises(RuntimeError):
                s.push(f, c, start=[0])                    # start during release
        assert s.slot_states() == states                   # nothing changed
        ys.append(s.push(f, c, start=start[h], stop=stop[h]).cpu().numpy())
        pres.append(s._last_pre.cpu().numpy())
    y, pre = np.concatenate(ys, 1), np.concatenate(pres, 1)
    dry, y_ref = expected(oracle, weights, voices, f0, control, pu, nz, K, F)
    judge("slots_after_misuse", y, pre, dry, y_ref, voices)
    assert s.idle_slots() == [0, 1, 2]
    tail = s.reverb_tail()
    assert tail.shape[0] == B and torch.isfinite(tail).all() and not tail[2].any()
    s.close()


def test_slot_large_batch(setup):
    """B = 1100 (beyond the recurrence workgroups the GPU holds at once), staggered starts: finite, check() passes, four sampled
    slots match the oracle"""
    model, oracle, weights = setup
    B, K, H = 1100, 2, 5
    F = H * K
    voices = {b: [(b % 3, 1 + b % 2)] for b in range(B)}
    start, stop = events(voices, B, H)
    g = torch.Generator().manual_seed(1100)
    f0 = (120 + 600 * torch.rand(B, 1, 1, generator=g)) * (1 + 0.03 * torch.randn(B, 1, F, generator=g))
    control = torch.randn(B, 2, F, generator=g)
    pu, nz = torch.rand(101, generator=g), torch.rand(128 * F - 1, generator=g)
    s = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda())
    y, pre = run(s, f0, control, K, H, start, stop)
    assert np.isfinite(y).all()
    s.check()
    pick = [0, 1, 548, 1099]
    sub = {i: voices[b] for i, b in enumerate(pick)}
    dry, y_ref = expected(oracle, weights, sub, f0[pick], control[pick], pu, nz, K, F)
    judge("slots_B1100", y[pick], pre[pick], dry, y_ref, sub)
    s.close()


LONG_VOICES = {0: [(0, 21), (23, 11)], 1: [(30, 3)], 2: []}


@pytest.fixture(scope="module")
def long_slot_runs(setup):
    """B = 3, K = 16, 35 hops = 560 frames (the ring position is 192 + 2048 h: hop 31 writes across index 65 536).  Slot 0: a
    voice of 336 frames - longer than the impulse response, so its own tail feeds its later samples through non-zero old parts -
    restarted at hop 23 while that tail rings and alive across the wrap; slot 1: a voice that starts before the wrap and stops
    after it; slot 2: never used, fed NaN / inf throughout.  Once eagerly, once through static_io / hop (graph replay)."""
    model, oracle, weights = setup
    B, K, H = 3, 16, 35
    start, stop = events(LONG_VOICES, B, H)
    f0, control, pu, nz = inputs(B, H * K, 35, LONG_VOICES, K)
    runs = {}
    for name, static in (("eager", False), ("replay", True)):
        s = model.stream(B, slots=True, phase_u=pu.cuda(), noise=nz.cuda(), graph=static)
        y, pre = run(s, f0, control, K, H, start, stop, static=static)
        s.check()
        tail = s.reverb_tail()
        runs[name] = dict(y=y, pre=pre, tail=tail.cpu().numpy(), graphs=len(s._graphs), idle=s.idle_slots())
        s.close()
    dry, y_ref = expected(oracle, weights, LONG_VOICES, f0, control, pu, nz, K, H * K)
    return runs, dry, y_ref, weights["reverb.ir"][0]


def test_slots_past_the_reverb_length_and_the_ring_wrap(long_slot_runs):
    """judge()'s bars over 71 680 samples per slot, the never-used slot exactly 0 throughout, and the output against the run's OWN
    dry signal through a float64 convolution (whole run, and the samples from the wrap on): what test_cpu_stream_long.py shows a
    dropped part, a late sample or a ring that loses its input at the wrap would miss by 8x .. 900x.
    Measured: own-pre reverb 1.2e-8 RMS over the run, 1.4e-8 from the wrap on; against the oracle pre 7.8e-8 max-abs, y 1.1e-7 RMS."""
    runs, dry, y_ref, ir = long_slot_runs
    r = runs["eager"]
    assert r["y"].shape == r["pre"].shape == (3, 128 * 560)
    e = reverb_errors(r["y"], r["pre"], None, ir)
    record("slots_long_B3_K16", **{f"own_{k}_rms_err": v for k, v in e.items()})
    print("slots long own-pre reverb", e, "pre", maxabs(r["pre"], dry), "y", rms(r["y"] - y_ref))
    judge("slots_long_B3_K16_vs_oracle", r["y"], r["pre"], dry, y_ref, LONG_VOICES)
    assert e["whole"] <= 1e-4 and e["after_wrap"] <= 1e-4, e
    assert r["tail"].shape[0] == 3 and np.isfinite(r["tail"]).all() and not r["tail"][2].any() and r["tail"][0].any()
    assert r["idle"] == [0, 1, 2]


def test_slots_past_the_wrap_graph_replay_bit_identical(long_slot_runs):
    runs = long_slot_runs[0]
    a, b = runs["eager"], runs["replay"]
    assert a["graphs"] == 0 and b["graphs"] == 1
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["pre"], b["pre"]) and np.array_equal(a["tail"], b["tail"])


def _rerun(env, *select):
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_stream_slots.py"), *select],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


@pytest.mark.skipif(os.environ.get("NWS_BACKEND") == "ctypes", reason="already the ctypes pass")
def test_slots_through_the_ctypes_binding():
    """every test of this file again through the torch-free ctypes binding of nws_stream_step_slots"""
    _rerun({"NWS_BACKEND": "ctypes"}, "-k", "not through_the and not older_launch_forms")


@pytest.mark.skipif(os.environ.get("NWS_BACKEND") == "ctypes" or os.environ.get("NWS_STREAM_FUSE_MLP") == "0",
                    reason="already a pass of its own")
def test_slots_in_older_launch_forms():
    """hops of one or two frames take the four-launch form by default; with its switches off the slot hop takes the seven-launch
    form, which must give the same parity (K = 1, 2 at B = 3 / 17) and the same captured-hop identity"""
    _rerun({"NWS_STREAM_FUSE_MLP": "0"}, "-k", "schedule_parity and (1-3 or 2-3 or 1-17 or 2-17) or graph_replay and 2")
    _rerun({"NWS_STREAM_SPLIT_REVERB": "0"}, "-k", "schedule_parity and (2-3 or 2-17)")
