"""GPU tests of the loudness stream (csrc/loudness_stream.hip, streaming.StreamLoudness / StreamControl).
Almost every check is an equality with the offline kernels: with the clip's own peak power as its fixed reference the stream is
nws_loudness bit for bit at any lag and chunking, so is the running reference at a lag of the whole clip, and at any lag a
running frame is the fixed stream at the reference that frame reports.  Against the float64 restatement the bar is the offline
kernel's own (tests/test_gpu_loudness.py): 2e-5 in normalised units.
The same file passes with NWS_BACKEND=ctypes (the ctypes binding instead of torch.ops)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import loudness_stream_restatement as ls
from conftest import ROOT
from test_gpu_loudness import _cases

pytestmark = pytest.mark.gpu

# (n_fft, hop, N)
CONFIGS = {
    "partial_tiles_odd_hop": (64, 37, 3001),       # 66 of 128 rows are bins, 82 frames: partial M-tile and frame tile
    "hop_not_pow2": (256, 100, 3001),
    "pipeline": (1024, 128, 4099),
    "largest_transform": (2048, 512, 30000),
    "shorter_than_a_frame": (1024, 128, 700),      # W < N < n_fft: both reflections meet in the flush
    "rings_wrap": (64, 16, 9000),                  # 563 frames in rings of 512
}


def _cuda(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return torch.from_numpy(x).cuda().reshape(-1, x.shape[-1])


@functools.lru_cache(maxsize=None)
def _clip(name):
    """noise under a rising and falling gain (the running reference keeps moving), the offline feature and the peak power: once"""
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import loudness_extraction as le
    n_fft, hop, N = CONFIGS[name]
    g = np.random.default_rng(sum(map(ord, name)))
    x = 0.2 * g.standard_normal(N) * np.interp(np.arange(N), [0, 0.3 * N, 0.7 * N, N], [0.05, 0.3, 1.0, 0.2])
    a = _cuda(x)
    return a, n_fft, hop, le.loudness_frames(a, n_fft, hop), le.peak_power(a, n_fft, hop)


def _chunkings(n, hop):
    irregular, at = [], 0
    while at < n:
        irregular.append(min(n - at, (37, 500, 129, 1)[len(irregular) % 4]))
        at += irregular[-1]
    hops = [hop] * (n // hop) + ([n % hop] if n % hop else [])
    return {"whole": ([n], True), "hops": (hops, True), "irregular": (irregular, True),
            "empty_final": ([1000] * (n // 1000) + ([n % 1000] if n % 1000 else []), False)}


def _run(a, n_fft, hop, lag, chunks, final_on_last=True, **kw):
    """push `chunks` of a (B, N) through a StreamLoudness -> (loudness, reference_power), per-push column counts, the stream"""
    from nws_amd.streaming import StreamLoudness
    s = StreamLoudness(a.shape[0], n_fft=n_fft, hop_length=hop, lag=lag, **kw)
    outs, at = [], 0
    for i, n in enumerate(chunks):
        outs.append(s.push(a[:, at:at + n], final=final_on_last and i == len(chunks) - 1))
        at += n
    if not final_on_last:
        outs.append(s.flush())
    assert at == a.shape[1]
    s.check()
    return tuple(torch.cat([o[i] for o in outs], dim=1) for i in range(2)), [o[0].shape[1] for o in outs], s


def _restated(a, n_fft, hop, lag, **kw):
    loud, ref = ls.stream(a[0].cpu().numpy().astype(np.float64), n_fft, hop, lag, **kw)
    return loud, ref


def test_peak_power_is_the_offline_reference():
    """the largest power of the float64 STFT, to the fp32 transform's precision (a sum of n_fft products: 1e-4 relative is
    n_fft 2^-24 with room); per row; refusals"""
    from nws_amd.data.utils import loudness_extraction as le
    for name in ("partial_tiles_odd_hop", "pipeline", "largest_transform"):
        a, n_fft, hop, _, peak = _clip(name)
        want = (ls.lo.stft_magnitude(a[0].cpu().numpy().astype(np.float64), n_fft, hop) ** 2).max()
        assert peak.shape == (1,) and peak.dtype == torch.float32 and abs(float(peak[0]) - want) <= 1e-4 * want, name
    a = _clip("pipeline")[0]
    rows = torch.cat([a, 0.1 * a, torch.zeros_like(a)]).contiguous()
    got = le.peak_power(rows, 1024, 128)
    assert torch.equal(got[:1], _clip("pipeline")[4]) and float(got[2]) == 0.0 and 0 < float(got[1]) < 0.011 * float(got[0])
    with pytest.raises(RuntimeError):
        le.peak_power(rows.cpu(), 1024, 128)
    with pytest.raises(RuntimeError):
        le.peak_power(rows[:, :512].contiguous(), 1024, 128)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fixed_at_the_clip_peak_equals_offline_bit_for_bit(name):
    """consequence 1: at any lag and any chunking"""
    a, n_fft, hop, offline, peak = _clip(name)
    T = offline.shape[1]
    assert T == 1 + a.shape[1] // hop and (name != "rings_wrap" or T == 563)
    for lag in (0, 4):
        for tag, (chunks, fin) in _chunkings(a.shape[1], hop).items():
            (loud, ref), counts, s = _run(a, n_fft, hop, lag, chunks, fin, reference=peak)
            assert loud.dtype == torch.float32 and loud.shape == (1, T) and sum(counts) == T
            assert torch.equal(loud, offline), (name, lag, tag, float((loud - offline).abs().max()))
            assert torch.equal(ref, peak.expand(T).unsqueeze(0))
            assert s.frames_out == T and s.samples_in == a.shape[1] and s.finished
    if name == "rings_wrap":            # named: the frames either side of the rings' length
        assert torch.equal(loud[:, 505:520], offline[:, 505:520])


@pytest.mark.parametrize("name", [n for n in CONFIGS if n != "rings_wrap"])
def test_running_at_a_lag_of_the_whole_clip_equals_offline_bit_for_bit(name):
    """consequence 2: nothing leaves before `final`, and the flush measures everything against M(T - 1), the clip's maximum"""
    a, n_fft, hop, offline, peak = _clip(name)
    T = offline.shape[1]
    assert T - 1 <= 255
    for tag, (chunks, fin) in _chunkings(a.shape[1], hop).items():
        (loud, ref), counts, _ = _run(a, n_fft, hop, 255, chunks, fin)
        assert sum(counts[:-1]) == 0 and counts[-1] == T, (tag, counts)
        assert torch.equal(loud, offline) and torch.equal(ref, peak.expand(T).unsqueeze(0)), (name, tag)


@pytest.mark.parametrize("lag", [0, 4])
def test_a_running_frame_is_the_fixed_stream_at_the_reference_it_reports(lag):
    """consequence 3 on a staircase of noise bursts: the reference climbs with the steps (and stays where the gain falls)"""
    g = np.random.default_rng(31)
    x = np.concatenate([gain * g.standard_normal(2000) for gain in (0.05, 0.2, 0.1, 0.5)])
    a = _cuda(x)
    chunks, fin = _chunkings(8000, 128)["irregular"]
    (loud, ref), _, _ = _run(a, 1024, 128, lag, chunks, fin)
    T = loud.shape[1]
    assert T == 63 and bool((ref[0, 1:] >= ref[0, :-1]).all()) and len(set(ref[0].tolist())) >= 4
    frames = (2, 12, 20, 33, 44, 60)
    assert len({float(ref[0, e]) for e in frames}) >= 3                  # spread over the steps
    for e in frames:
        (fixed, fref), _, _ = _run(a, 1024, 128, lag, [8000], reference=float(ref[0, e]))
        assert torch.equal(fixed[:, e], loud[:, e]) and float(fref[0, e]) == float(ref[0, e]), (lag, e)
    # the reference of frame e is the running maximum of the frames' peaks up to e + lag (against the restatement: fp32 powers)
    want_loud, want_ref = _restated(a, 1024, 128, lag)
    assert np.allclose(ref[0].cpu().numpy(), want_ref, rtol=1e-4, atol=0)
    assert np.abs(loud[0].cpu().numpy() - want_loud).max() <= 2e-5


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chunking_does_not_change_a_bit(name):
    """consequence 4, running reference: lags 0 / 4 / 8 x the four chunkings; hop by hop every push releases E's difference"""
    from nws_amd import _lib
    a, n_fft, hop, offline, peak = _clip(name)
    ch = _chunkings(a.shape[1], hop)
    for lag in (0, 4, 8):
        want, want_counts, _ = _run(a, n_fft, hop, lag, *ch["whole"])
        per_push = None
        for tag in ("hops", "irregular", "empty_final"):
            got, counts, _ = _run(a, n_fft, hop, lag, *ch[tag])
            for g, w in zip(got, want):
                assert torch.equal(g, w), (name, lag, tag)
            assert sum(counts) == sum(want_counts) == offline.shape[1]
            per_push = counts if tag == "hops" else per_push
        seen, prev = 0, 0
        for n, m in zip(ch["hops"][0][:-1], per_push[:-1]):
            seen += n
            e = int(_lib.lib().nws_loudness_stream_emitted(seen, n_fft, hop, lag, 0))
            assert m == e - prev, (name, lag, seen)
            prev = e
        # consequence 5: once e + lag has reached the clip's loudest frame the frames are the offline ones
        reached = int((want[1][0] == peak[0]).nonzero()[0]) if bool((want[1][0] == peak[0]).any()) else None
        assert reached is not None and torch.equal(want[0][:, reached:], offline[:, reached:]), (name, lag)
        if name == "rings_wrap":
            assert reached < 500 and torch.equal(want[0][:, 505:520], offline[:, 505:520])


@pytest.mark.parametrize("name", ["silence_then_click", "all_zero"])
def test_silence_and_a_click(name):
    """digital silence in front of the click has P = 0 against M = 0: 0 dB, 1.0 normalised, until the click is lag frames away
    (what floor_power is for); all_zero stays there, as offline"""
    from nws_amd.data.utils import loudness_extraction as le
    x, n_fft, hop = _cases()[name]
    a = _cuda(x)
    offline, peak = le.loudness_frames(a, n_fft, hop), le.peak_power(a, n_fft, hop)
    ch = _chunkings(a.shape[1], hop)
    (fixed, _), _, _ = _run(a, n_fft, hop, 4, *ch["irregular"], reference=peak)
    assert torch.equal(fixed, offline)
    (loud, ref), _, _ = _run(a, n_fft, hop, 4, *ch["irregular"])
    (loud_h, ref_h), _, _ = _run(a, n_fft, hop, 4, *ch["hops"])
    assert torch.equal(loud, loud_h) and torch.equal(ref, ref_h)
    want_loud, want_ref = _restated(a, n_fft, hop, 4)
    assert np.abs(loud[0].cpu().numpy() - want_loud).max() <= 2e-5
    if name == "all_zero":
        assert float(peak[0]) == 0.0 and bool((ref == 0).all()) and bool((loud == 1.0).all()) and torch.equal(loud, offline)
    else:
        first, reached = int((ref[0] > 0).nonzero()[0]), int((ref[0] == peak[0]).nonzero()[0])
        assert first == 3000 // hop - (n_fft // 2) // hop + 1 - 4            # the first frame that holds the click, four frames early
        assert first < reached <= 3000 // hop + 1 - 4                        # the click at the window's centre, four frames early
        assert bool((loud[0, :first] == 1.0).all()) and torch.equal(loud[:, reached:], offline[:, reached:])
        # a floor: the silence in front is measured against it instead
        (floored, fref), _, _ = _run(a, n_fft, hop, 4, *ch["irregular"], floor_power=1.0)
        assert bool((fref[0, :first] == 1.0).all()) and float(floored[0, :first].max()) < 0.5


def test_batch_rows_equal_their_single_row_bits():
    a = _clip("pipeline")[0]
    rows = torch.cat([a, 0.03 * a, 0.5 * a.flip(1)]).contiguous()
    chunks, fin = _chunkings(4099, 128)["irregular"]
    got, _, _ = _run(rows, 1024, 128, 4, chunks, fin)
    assert got[0].shape == (3, 33) and len({float(v) for v in got[1][:, -1]}) == 3
    floors = torch.tensor([0.0, 5.0, 1e-3], device="cuda")
    got_f, _, _ = _run(rows, 1024, 128, 4, chunks, fin, floor_power=floors)
    for b in range(3):
        one, _, _ = _run(rows[b:b + 1].contiguous(), 1024, 128, 4, chunks, fin)
        one_f, _, _ = _run(rows[b:b + 1].contiguous(), 1024, 128, 4, chunks, fin, floor_power=float(floors[b]))
        for g, w in zip(got + got_f, one + one_f):
            assert torch.equal(g[b:b + 1], w), b


def test_the_step_that_computes_frame_zero_at_the_largest_chunk_stays_inside_its_scratch():
    """from n_seen = W a step of 256 hops computes 257 frames, one more than any later step: the scratch of
    nws_loudness_stream_workspace_bytes holds them (a pattern behind it stays intact) and the frames are the offline ones"""
    from nws_amd import _lib
    from nws_amd.data.utils import loudness_extraction as le
    from nws_amd.streaming import StreamLoudness
    L = _lib.lib()
    n = 256 * 128
    a = _cuda(0.2 * np.random.default_rng(77).standard_normal(512 + n + 700) * np.linspace(0.1, 1.0, 512 + n + 700))
    offline, peak = le.loudness_frames(a, 1024, 128), le.peak_power(a, 1024, 128)
    s = StreamLoudness(1, lag=0, reference=peak)
    assert s.max_chunk == n
    s.push(a[:, :512])
    assert s.frames_out == 0
    need = L.nws_loudness_stream_workspace_bytes(1, n, 1024, 128, 0)
    assert need == ls.workspace_bytes(1, 257)
    ws = torch.full((need + 16384,), 0xA5, dtype=torch.uint8, device="cuda")
    m = 257
    loud, ref = torch.full((1, m + 3), float("nan"), device="cuda"), torch.full((1, m + 3), float("nan"), device="cuda")
    x = a[:, 512:512 + n].contiguous()
    rc = L.nws_loudness_stream_step(s._state.data_ptr(), s._state.numel(), x.data_ptr(), 1, n, 512, 1024, 128, 0, s._dft.data_ptr(), 1e-5, 80.0,
                                    1, 0, loud.data_ptr(), ref.data_ptr(), m + 3, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((ws[need:] == 0xA5).all())
    assert torch.equal(loud[:, :m], offline[:, :m]) and bool(torch.isnan(loud[:, m:]).all()) and bool(torch.isnan(ref[:, m:]).all())
    s._n_seen, s._emitted = 512 + n, m
    s.check()
    rest = s.push(a[:, 512 + n:], final=True)[0]
    assert torch.equal(rest, offline[:, m:])


@pytest.mark.parametrize("name", ["partial_tiles_odd_hop", "pipeline", "largest_transform", "shorter_than_a_frame"])
def test_running_and_floored_running_against_the_restatement(name):
    """2e-5 normalised: the bar tests/test_gpu_loudness.py holds the offline kernel to (the same arithmetic); the reference power
    to 1e-4 relative (an fp32 sum of n_fft products), and exactly the floor where nothing louder has been heard"""
    a, n_fft, hop, _, peak = _clip(name)
    chunks, fin = _chunkings(a.shape[1], hop)["irregular"]
    floor = 0.2 * float(peak[0])
    for lag in (0, 4, 8):
        for kw in (dict(), dict(floor_power=floor)):
            (loud, ref), _, _ = _run(a, n_fft, hop, lag, chunks, fin, **kw)
            want_loud, want_ref = _restated(a, n_fft, hop, lag, initial=float(np.float32(kw.get("floor_power", 0.0))))
            err = float(np.abs(loud[0].cpu().numpy() - want_loud).max())
            print(name, "lag", lag, kw, "max |stream - restatement|", err)
            assert err <= 2e-5, (name, lag, kw, err)
            assert np.allclose(ref[0].cpu().numpy(), want_ref, rtol=1e-4, atol=0)
            if kw:
                held = want_ref == np.float32(floor)
                assert (held.any() or name == "shorter_than_a_frame") and bool((ref[0].cpu().numpy()[held] == np.float32(floor)).all())


def test_unnormalised_and_a_reference_below_the_signal():
    """without `normalise` the values are dB; a fixed reference below the signal gives values above 0 dB, not clipped"""
    a, n_fft, hop, offline, peak = _clip("pipeline")
    (db, _), _, _ = _run(a, n_fft, hop, 4, [4099], reference=peak, normalise=False)
    assert torch.allclose((db + 80) / 80, offline, atol=1e-6) and float(db.max()) <= 0.0
    (hot, _), _, _ = _run(a, n_fft, hop, 4, [4099], reference=1e-4 * float(peak[0]), normalise=False)
    (hot_n, _), _, _ = _run(a, n_fft, hop, 4, [4099], reference=1e-4 * float(peak[0]))
    assert float(hot.max()) > 0.0 and float(hot_n.max()) > 1.0


def test_lifecycle_counters_and_bad_input():
    from nws_amd.streaming import StreamLoudness
    a = _clip("pipeline")[0]
    s = StreamLoudness(1, lag=4)
    assert s.latency_samples == 512 + 4 * 128 and s.frames_out == 0 and s.samples_in == 0 and s.max_chunk == 256 * 128
    first = s.push(a[:, :2000])
    assert s.samples_in == 2000 and s.frames_out == first[0].shape[1] == 1 + (2000 - 512) // 128 - 4
    rest = s.push(a[0, 2000:], final=True)                 # a (n,) chunk is a row of a one-row stream
    assert s.frames_out == 33 and first[0].shape[1] + rest[0].shape[1] == 33 and s.finished
    s.check()
    with pytest.raises(RuntimeError, match="finished"):
        s.push(a[:, :128])
    with pytest.raises(RuntimeError, match="finished"):
        s.flush()
    s.reset()
    assert s.frames_out == 0 and s.samples_in == 0 and not s.finished
    again = s.push(a[:, :2000]), s.push(a[:, 2000:], final=True)
    for i in range(2):
        assert torch.equal(again[0][i], first[i]) and torch.equal(again[1][i], rest[i])      # the running maximum started over
    s.reset()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.push(a.cpu())
    with pytest.raises(RuntimeError, match="empty chunk"):
        s.push(a[:, :0])
    with pytest.raises(RuntimeError, match="cannot end"):
        s.push(a[:, :512], final=True)
    with pytest.raises(RuntimeError, match="expected a"):
        s.push(torch.zeros(2, 128, device="cuda"))
    s.check()                                              # none of them moved the stream
    with pytest.raises(RuntimeError, match="lag"):
        StreamLoudness(1, lag=256)
    with pytest.raises(RuntimeError, match="unsupported"):
        StreamLoudness(1, n_fft=4096)
    with pytest.raises(RuntimeError, match="unsupported"):
        StreamLoudness(1, n_fft=1024, hop_length=1)
    with pytest.raises(RuntimeError, match="reference"):
        StreamLoudness(1, reference="clip")
    with pytest.raises(RuntimeError, match="floor_power"):
        StreamLoudness(1, reference=1.0, floor_power=1.0)
    with pytest.raises(RuntimeError, match=">= 0"):
        StreamLoudness(1, reference=-1.0)
    with pytest.raises(RuntimeError, match="powers"):
        StreamLoudness(2, reference=torch.ones(3))
    # chunks above the maximum are split
    s2 = StreamLoudness(1, n_fft=64, hop_length=16, lag=4)
    x = _clip("rings_wrap")[0]
    assert x.shape[1] > s2.max_chunk
    whole_push = s2.push(x, final=True)
    s2.reset()
    parts = s2.push(x[:, :5000]), s2.push(x[:, 5000:], final=True)
    for i in range(2):
        assert torch.equal(whole_push[i], torch.cat([parts[0][i], parts[1][i]], dim=1))


def test_refusals_leave_state_and_outputs_untouched():
    from nws_amd import _lib, engine
    from nws_amd.streaming import StreamLoudness
    L = _lib.lib()
    a = _clip("pipeline")[0]
    s = StreamLoudness(2, lag=4)
    a2 = torch.cat([a, 0.3 * a.flip(1)]).contiguous()
    s.push(a2[:, :2048])
    torch.cuda.synchronize()
    state0 = s._state.clone()
    loud, ref = torch.full((2, 16), float("nan"), device="cuda"), torch.full((2, 16), float("nan"), device="cuda")
    x = a2[:, 2048:2304].contiguous()
    ws = torch.empty(L.nws_loudness_stream_workspace_bytes(2, 256, 1024, 128, 1), dtype=torch.uint8, device="cuda")
    need = L.nws_loudness_stream_state_bytes(2, 1024, 128)
    assert need == s._state.numel()

    def step(state=s._state.data_ptr(), size=need, xp=x.data_ptr(), B=2, n=256, n_seen=2048, n_fft=1024, hop=128, lag=4, dft=s._dft.data_ptr(),
             amin=1e-5, final=0, lp=loud.data_ptr(), rp=ref.data_ptr(), stride=16, wsp=ws.data_ptr(), ws_bytes=ws.numel()):
        return L.nws_loudness_stream_step(state, size, xp, B, n, n_seen, n_fft, hop, lag, dft, amin, 80.0, 1, final, lp, rp, stride, wsp, ws_bytes,
                                          torch.cuda.current_stream().cuda_stream)

    bad_arg = [dict(state=None), dict(dft=None), dict(lp=None), dict(rp=None), dict(wsp=None), dict(xp=None), dict(B=0), dict(n=-1), dict(n=0),
               dict(n=12, n_seen=500, final=1), dict(stride=1), dict(n=0, final=1, stride=7), dict(size=need - 1),
               dict(ws_bytes=L.nws_loudness_stream_workspace_bytes(2, 256, 1024, 128, 0) - 1), dict(lag=-1), dict(lag=256), dict(n_seen=-1),
               dict(amin=0.0)]
    unsupported = [dict(n_fft=4096), dict(n=256 * 128 + 1), dict(B=65536), dict(hop=1)]
    for kw in bad_arg:
        assert step(**kw) == -2, kw
    for kw in unsupported:
        assert step(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(s._state, state0) and bool(torch.isnan(loud).all()) and bool(torch.isnan(ref).all())
    # a step whose n_seen is not the stream's launches, and changes nothing either
    assert step(n_seen=1920) == 0
    torch.cuda.synchronize()
    assert torch.equal(s._state, state0) and bool(torch.isnan(loud).all()) and bool(torch.isnan(ref).all())
    # a valid call right after gives the op's bits
    twin = StreamLoudness(2, lag=4)
    twin._state.copy_(state0)
    twin._n_seen, twin._emitted = 2048, s.frames_out
    want = twin.push(x)
    assert step() == 0
    torch.cuda.synchronize()
    m = want[0].shape[1]
    assert m == 2 and torch.equal(loud[:, :m], want[0]) and torch.equal(ref[:, :m], want[1])
    assert bool(torch.isnan(loud[:, m:]).all()) and torch.equal(s._state, twin._state)
    # a stream that has had `final` accepts nothing until the next reset
    twin.push(a2[:, 2304:], final=True)
    torch.cuda.synchronize()
    done = twin._state.clone()
    loud.fill_(float("nan"))
    assert step(state=twin._state.data_ptr(), n_seen=4099) == 0
    torch.cuda.synchronize()
    assert torch.equal(twin._state, done) and bool(torch.isnan(loud).all())
    # the binding refuses what it can see, with a text
    b = engine.binding()
    twin.reset()
    outs = (torch.empty(2, 4, device="cuda"), torch.empty(2, 4, device="cuda"))
    args = (twin._state, s._dft, 1024, 128)
    with pytest.raises(RuntimeError, match="lag"):
        b.loudness_stream_step(*args, 300, x, 0, False, 1e-5, 80.0, True, *outs)
    with pytest.raises(RuntimeError, match="dft"):
        b.loudness_stream_step(twin._state, s._dft[:-4], 1024, 128, 4, x, 0, False, 1e-5, 80.0, True, *outs)
    with pytest.raises(RuntimeError, match="state"):
        b.loudness_stream_step(twin._state[:-8], s._dft, 1024, 128, 4, x, 0, False, 1e-5, 80.0, True, *outs)
    with pytest.raises(RuntimeError, match="reference_power"):
        b.loudness_stream_step(*args, 4, x, 0, False, 1e-5, 80.0, True, outs[0], outs[1].double())
    with pytest.raises(RuntimeError, match=">= 2"):
        b.loudness_stream_step(*args, 4, x, 2048, False, 1e-5, 80.0, True, *[o[:, :1].contiguous() for o in outs])
    with pytest.raises(RuntimeError, match="amin"):
        b.loudness_stream_step(*args, 4, x, 0, False, 0.0, 80.0, True, *outs)
    with pytest.raises(RuntimeError, match="initial_power"):
        b.loudness_stream_reset(twin._state, 2, 1024, 128, torch.zeros(3, device="cuda"), True)
    with pytest.raises(RuntimeError, match="too small"):
        b.loudness_stream_reset(twin._state[:-8], 2, 1024, 128, torch.zeros(2, device="cuda"), True)
    twin.check()


# ---- StreamControl -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    import nws_amd as nws
    nws.ensure_default_config()
    model = nws.NeuralWaveshaping.load_from_checkpoint(os.path.join(ROOT, "tests", "golden", "weights_vn.npz")).to("cuda:0").eval()
    model.newt = nws.FastNEWT(model.newt)
    return model


def _tone(seconds, sr=16000, f=220.0):
    t = np.arange(int(sr * seconds)) / sr
    return (0.3 * np.sin(2 * np.pi * f * t) * np.minimum(1.0, 10 * t)).astype(np.float32)


def test_stream_control_is_make_control_of_the_two_streams_frames():
    from nws_amd import checkpoint as ck
    from nws_amd.streaming import StreamControl, StreamF0, StreamLoudness
    model = _model()
    a = _cuda(np.stack([_tone(0.5), 0.2 * _tone(0.5, f=330.0)]))
    mean, std = np.array([300.0, 0.4]), np.array([150.0, 0.25])
    sc = StreamControl(model, 2, lag=4, mean=mean, std=std, octave_shift=1)
    sf, sl = StreamF0(2, lag=4), StreamLoudness(2, lag=4)
    assert sc.latency_samples == 512 + 4 * 128
    chunks, fin = _chunkings(a.shape[1], 128)["irregular"]
    at, total = 0, 0
    for i, n in enumerate(chunks):
        last = i == len(chunks) - 1
        f0, control = sc.push(a[:, at:at + n], final=last)
        f0_frames, loud = sf.push(a[:, at:at + n], final=last)[0], sl.push(a[:, at:at + n], final=last)[0]
        m = f0_frames.shape[1]
        assert loud.shape[1] == m and f0.shape == (2, 1, m) and control.shape == (2, 2, m) and f0.dtype == control.dtype == torch.float32
        want_f0, want_c = ck.make_control(f0_frames.cpu().numpy().astype(np.float64) * 2.0, loud.cpu().numpy(), mean, std)
        assert torch.equal(f0.cpu(), want_f0) and torch.equal(control.cpu(), want_c), i
        at, total = at + n, total + m
    assert total == 1 + a.shape[1] // 128 and sc.finished
    sc.check()
    sc.reset()
    f0, control = sc.push(a[:, :3000])
    assert f0.shape[2] == 1 + (3000 - 512) // 128 - 4 and not sc.finished
    flushed = sc.flush()
    assert flushed[0].shape[2] == 1 + 3000 // 128 - f0.shape[2]


def test_one_chunk_through_stream_control_and_the_model_stream_renders_audio():
    from nws_amd.streaming import StreamControl
    model = _model()
    a = _cuda(_tone(0.5))
    sc = StreamControl(model, 1, lag=4, mean=[300.0, 0.4], std=[150.0, 0.25])
    f0, control = sc.push(a, final=True)
    assert f0.shape == (1, 1, 63)
    with torch.no_grad():
        y = model.stream(1).push(f0, control, final=True)
    assert y.shape == (1, 63 * 128) and bool(torch.isfinite(y).all()) and float(y.pow(2).mean().sqrt()) > 0


# ---- scripts -------------------------------------------------------------------------------------------------------------
def _script(name, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name), *args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_timbre_transfer_with_streamed_loudness_writes_the_plain_runs_wav(tmp_path):
    """--loudness-reference clip at lag 4, and the running reference at a lag of the whole clip; the runs fix the model's two
    random draws with the same --seed"""
    x = _tone(0.5)
    src = str(tmp_path / "in.wav")
    wavfile.write(src, 16000, x)
    runs = {"plain": [], "clip": ["--stream-loudness", "4", "--loudness-reference", "clip", "--chunk", "300"],
            "running": ["--stream-loudness", "255", "--chunk", "300"]}
    data = {}
    for tag, extra in runs.items():
        dst = str(tmp_path / (tag + ".wav"))
        _script("timbre_transfer.py", src, dst, "--use-fastnewt", "--seed", "1", *extra)
        with open(dst, "rb") as f:
            data[tag] = f.read()
    assert len(data["plain"]) > 4 * x.size                 # float32 samples of the input's length behind the header
    assert data["clip"] == data["plain"] and data["running"] == data["plain"]


def test_live_transfer_renders_a_tone_and_repeats_itself_with_a_seed(tmp_path):
    x = _tone(1.5)
    src = str(tmp_path / "in.wav")
    wavfile.write(src, 16000, x)
    data = []
    for tag in ("a", "b"):
        dst = str(tmp_path / (tag + ".wav"))
        out = _script("live_transfer.py", src, dst, "--use-fastnewt", "--seed", "5", "--chunk", "300", "--lag", "4")
        assert "latency of the chain 1024 samples at 16000 Hz + 64 samples at 16000 Hz = 68.0 ms" in out
        sr, y = wavfile.read(dst)
        assert sr == 16000 and y.dtype == np.float32 and y.shape == (x.size,) and np.isfinite(y).all() and float(np.sqrt(np.mean(y * y))) > 0
        with open(dst, "rb") as f:
            data.append(f.read())
    assert data[0] == data[1]
