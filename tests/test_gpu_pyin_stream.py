"""GPU tests of the fixed-lag pYIN stream (csrc/pyin_stream.hip, streaming.StreamF0).  Almost every check is an
equality with the offline kernels: a lag of the whole clip is nws_pyin bit for bit whatever the chunking, and at any lag the
streamed state of frame e is the offline decode of the first e + lag + 1 frames, read at e."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import pyin_restatement as pr
from conftest import ROOT
from test_gpu_pyin import _cases, _kw

pytestmark = pytest.mark.gpu

RING = 512


def _signal(name):
    cs = _cases()
    if name == "long_4s":
        return cs["long_10s"][0][:4 * 16000], {}
    if name == "long_5s":                                  # 626 frames: the rings of 512 frames wrap
        return cs["long_10s"][0][:5 * 16000], {}
    return cs[name]


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().reshape(-1, x.shape[-1])


@functools.lru_cache(maxsize=None)
def _offline(name):
    """the offline extractor on the whole signal + its observations (for decodes of a prefix): once per signal"""
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import f0_extraction as fe
    x, kw = _signal(name)
    c = pr.config(**kw)
    a = _cuda(x)
    f0, vp, states = fe.pyin_frames(a, **_kw(c))
    obs = fe.pyin_observe(fe.pyin_cmnd(a, **_kw(c)), **_kw(c))
    return c, a, (f0, vp, states), obs


def _chunkings(n, hop):
    irregular, at = [], 0
    while at < n:
        irregular.append(min(n - at, (37, 500, 129, 1)[len(irregular) % 4]))
        at += irregular[-1]
    hops = [hop] * (n // hop) + ([n % hop] if n % hop else [])
    return {"whole": ([n], True), "hops": (hops, True), "irregular": (irregular, True),
            "empty_final": ([1000] * (n // 1000) + ([n % 1000] if n % 1000 else []), False)}


def _run(a, c, lag, chunks, final_on_last=True, stream=None, fill=None):
    """push `chunks` of a (B, N) through a StreamF0 -> the concatenated (f0, voiced_prob, states) + per-push column counts"""
    from nws_amd.streaming import StreamF0
    s = stream if stream is not None else StreamF0(a.shape[0], lag=lag, fill_unvoiced=fill, **_kw(c))
    outs, at = [], 0
    for i, n in enumerate(chunks):
        outs.append(s.push(a[:, at:at + n], final=final_on_last and i == len(chunks) - 1))
        at += n
    if not final_on_last:
        outs.append(s.flush())
    assert at == a.shape[1]
    s.check()
    return tuple(torch.cat([o[i] for o in outs], dim=1) for i in range(3)), [o[0].shape[1] for o in outs], s


def _prefix_state(name, e, lag):
    """offline decode of the frames 0 .. e + lag, read at frame e"""
    from nws_amd.data.utils import f0_extraction as fe
    c, _, _, obs = _offline(name)
    cut = [o[:, :e + lag + 1].contiguous() for o in obs]
    states, _ = fe.pyin_viterbi(*cut, **_kw(c))
    return int(states[0, e])


def _check_against_offline_forward(name, lag, got_states, frames):
    """frames e with e + lag computed before the end: the prefix decode; the frames after them: the whole-signal decode"""
    from nws_amd import _lib
    c, a, whole, _ = _offline(name)
    T = whole[2].shape[1]
    F = int(_lib.lib().nws_pyin_stream_frames(a.shape[1], c.sr, c.fmin, c.fmax, c.frame_length, c.hop, 0))
    assert got_states.shape == (1, T) and 0 < F <= T
    for e in frames:
        if e + lag <= F - 1:
            assert int(got_states[0, e]) == _prefix_state(name, e, lag), (name, lag, e)
    tail = max(0, F - lag)
    assert torch.equal(got_states[:, tail:], whole[2][:, tail:]), (name, lag)


@pytest.mark.parametrize("name", ["short_600", "odd_length_4099", "frame_256_hop_100", "hop_64"])
def test_a_lag_of_the_whole_clip_equals_offline_bit_for_bit(name):
    c, a, whole, _ = _offline(name)
    T = whole[0].shape[1]
    assert T - 1 <= 255
    for tag, (chunks, final_on_last) in _chunkings(a.shape[1], c.hop).items():
        got, counts, s = _run(a, c, 255, chunks, final_on_last)
        assert sum(counts[:-1]) == 0 and counts[-1] == T, (tag, counts)          # nothing leaves before `final`
        for g, w, what in zip(got, whole, ("f0", "voiced_prob", "states")):
            assert g.dtype == w.dtype and torch.equal(g, w), (name, tag, what)
        assert s.frames_out == T and s.samples_in == a.shape[1] and s.finished


@pytest.mark.parametrize("name", ["frame_block_plus_one", "hop_64"])
@pytest.mark.parametrize("lag", [0, 1, 4, 8])
def test_any_lag_is_the_offline_forward_pass(name, lag):
    c, a, whole, _ = _offline(name)
    T = whole[0].shape[1]
    chunks, fin = _chunkings(a.shape[1], c.hop)["irregular"]
    got, _, _ = _run(a, c, lag, chunks, fin)
    frames = sorted({0, 1, T // 5, T // 2, (3 * T) // 4, max(0, T - lag - 6)})
    assert len(frames) == 6
    _check_against_offline_forward(name, lag, got[2], frames)
    # voiced_prob is the offline one delayed like the states; f0 is the table's value of the state's bin
    assert torch.equal(got[1], whole[1])
    from nws_amd.data.utils import f0_extraction as fe
    f0_of_bin = fe._table((c.sr, c.fmin, c.fmax, c.frame_length, c.hop), a.device)[-c.n_bins:]      # the table's last part
    assert torch.equal(got[0], f0_of_bin[(got[2] % c.n_bins).long()].float())
    assert abs(float(f0_of_bin[120]) - c.fmin * 2.0) < 1e-9


@pytest.mark.parametrize("name", ["odd_length_4099", "frame_256_hop_100"])
def test_chunking_does_not_change_a_bit_at_small_lags(name):
    c, a, _, _ = _offline(name)
    ch = _chunkings(a.shape[1], c.hop)
    for lag in (0, 4, 8):
        ref, ref_counts, _ = _run(a, c, lag, *ch["whole"])
        per_push = None
        for tag in ("hops", "irregular", "empty_final"):
            got, counts, _ = _run(a, c, lag, *ch[tag])
            for g, w in zip(got, ref):
                assert torch.equal(g, w), (name, lag, tag)
            assert sum(counts) == sum(ref_counts)
            per_push = counts if tag == "hops" else per_push
        # hop by hop: every push but the last releases E's difference
        seen, prev = 0, 0
        from nws_amd import _lib
        for n, m in zip(ch["hops"][0][:-1], per_push[:-1]):
            seen += n
            e = int(_lib.lib().nws_pyin_stream_emitted(seen, c.sr, c.fmin, c.fmax, c.frame_length, c.hop, lag, 0))
            assert m == e - prev, (name, lag, seen)
            prev = e


@pytest.mark.parametrize("name,frames", [("long_4s", (0, 250, 495, 496, 500)), ("long_5s", (250, 505, 511, 512, 513, 620))])
def test_long_streams_and_the_rings_wrap(name, frames):
    """long_4s: 501 frames fill the rings of 512 frames almost completely; long_5s: 626 frames wrap them"""
    c, a, whole, _ = _offline(name)
    N = a.shape[1]
    assert whole[0].shape[1] == 1 + N // 128 and (name != "long_5s" or whole[0].shape[1] > RING + 100)
    small = [128] * (N // 128) + ([N % 128] if N % 128 else [])
    big = [256 * 128] * (N // (256 * 128)) + ([N % (256 * 128)] if N % (256 * 128) else [])
    got_small, _, _ = _run(a, c, 4, small)
    got_big, counts, _ = _run(a, c, 4, big)
    assert counts[0] == 256 - 4 - 3                       # 32 768 samples: frames 0 .. 252 computed, four held back
    for g, w in zip(got_small, got_big):
        assert torch.equal(g, w)
    _check_against_offline_forward(name, 4, got_small[2], frames)
    # a lag as long as the rings allow still equals offline where the clip is short enough for it: the last 256 frames
    got, _, _ = _run(a, c, 255, big)
    _check_against_offline_forward(name, 255, got[2], [f for f in frames if f + 255 < whole[0].shape[1]][:2])


def test_batch_rows_equal_their_single_row_bits():
    cs = _cases()
    rows = np.stack([cs["odd_length_4099"][0], cs["frame_block_plus_one"][0][:4099], cs["white_noise"][0][:4099]])
    a = _cuda(rows)
    c = pr.config()
    chunks, fin = _chunkings(4099, c.hop)["irregular"]
    got, _, _ = _run(a, c, 4, chunks, fin)
    assert got[0].shape == (3, 33)
    for b in range(3):
        one, _, _ = _run(a[b:b + 1].contiguous(), c, 4, chunks, fin)
        for g, w in zip(got, one):
            assert torch.equal(g[b:b + 1], w), b


def test_lag_four_agrees_with_offline_on_the_cpu_tests_signals():
    """voiced flags equal on >= 99 % of the frames, bins equal on >= 99 % of the frames voiced in both (the restatement gives 100 %;
    the cap keeps a one-frame tie in silence from failing the run)"""
    for name in _cases():
        name = "long_4s" if name == "long_10s" else name
        c, a, whole, _ = _offline(name)
        N = a.shape[1]
        chunks = [4096] * (N // 4096) + ([N % 4096] if N % 4096 else [])
        got, _, _ = _run(a, c, 4, chunks)
        v_off, v_lag = whole[2][0] < c.n_bins, got[2][0] < c.n_bins
        both = v_off & v_lag
        flags = float((v_off == v_lag).double().mean())
        bins = float((got[2][0][both] == whole[2][0][both]).double().mean()) if bool(both.any()) else 1.0
        print(name, "frames", whole[2].shape[1], "voiced flags equal", flags, "bins equal where both voiced", bins)
        assert flags >= 0.99 and bins >= 0.99, (name, flags, bins)


def test_lifecycle_counters_and_bad_input():
    from nws_amd.streaming import StreamF0
    c, a, whole, _ = _offline("odd_length_4099")
    s = StreamF0(1, lag=4)
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
    for i in range(3):
        assert torch.equal(again[0][i], first[i]) and torch.equal(again[1][i], rest[i])
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
        StreamF0(1, lag=256)
    with pytest.raises(RuntimeError, match="unsupported"):
        StreamF0(1, frame_length=4096)
    # fill_unvoiced as offline's fill_na; chunks above the maximum are split
    filled, _, _ = _run(a, c, 4, [4099], fill=0.0)
    plain, _, _ = _run(a, c, 4, [4099])
    unv = plain[2] >= c.n_bins
    assert torch.equal(filled[2], plain[2]) and torch.all(filled[0][unv] == 0) and torch.equal(filled[0][~unv], plain[0][~unv])
    s2 = StreamF0(1, lag=4, hop_length=64)
    x = _cuda(np.tile(_cases()["hop_64"][0], 4))           # 19 200 samples > 256 * 64
    assert x.shape[1] > s2.max_chunk
    whole_push = s2.push(x, final=True)
    s2.reset()
    parts = s2.push(x[:, :9000]), s2.push(x[:, 9000:], final=True)
    for i in range(3):
        assert torch.equal(whole_push[i], torch.cat([parts[0][i], parts[1][i]], dim=1))


def test_refusals_leave_state_and_outputs_untouched():
    from nws_amd import _lib, engine
    from nws_amd.data.utils import f0_extraction as fe
    from nws_amd.streaming import StreamF0
    L = _lib.lib()
    c, a, _, _ = _offline("odd_length_4099")
    cfg = (c.sr, c.fmin, c.fmax, c.frame_length, c.hop)
    s = StreamF0(2, lag=4)
    a2 = torch.cat([a, a.flip(1)]).contiguous()
    s.push(a2[:, :2048])
    torch.cuda.synchronize()
    state0 = s._state.clone()
    table = fe._table(cfg, a.device)
    f0 = torch.full((2, 16), float("nan"), device="cuda")
    vp = torch.full((2, 16), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((2, 16), -7, dtype=torch.int32, device="cuda")
    x = a2[:, 2048:2304].contiguous()
    ws = torch.empty(L.nws_pyin_stream_workspace_bytes(2, 256, *cfg, 1), dtype=torch.uint8, device="cuda")
    need = L.nws_pyin_stream_state_bytes(2, *cfg)
    assert need == s._state.numel()

    def step(state=s._state.data_ptr(), size=need, xp=x.data_ptr(), B=2, n=256, n_seen=2048, cfg=cfg, lag=4, tb=table.data_ptr(), final=0,
             f0p=f0.data_ptr(), vpp=vp.data_ptr(), stp=st.data_ptr(), stride=16, wsp=ws.data_ptr(), ws_bytes=ws.numel()):
        return L.nws_pyin_stream_step(state, size, xp, B, n, n_seen, *cfg, lag, tb, final, 0, 0.0, f0p, vpp, stp, stride, wsp, ws_bytes,
                                      torch.cuda.current_stream().cuda_stream)

    bad_arg = [dict(state=None), dict(tb=None), dict(f0p=None), dict(vpp=None), dict(stp=None), dict(wsp=None), dict(xp=None), dict(B=0),
               dict(n=-1), dict(n=0), dict(n=12, n_seen=500, final=1), dict(stride=1), dict(n=0, final=1, stride=7), dict(size=need - 1),
               dict(ws_bytes=L.nws_pyin_stream_workspace_bytes(2, 256, *cfg, 0) - 1), dict(lag=-1), dict(lag=256), dict(n_seen=-1)]
    unsupported = [dict(cfg=(16000.0, 65.0, 2093.0, 4096, 128)), dict(n=256 * 128 + 1), dict(B=65536), dict(cfg=(16000.0, 65.0, 2093.0, 1024, 1))]
    for kw in bad_arg:
        assert step(**kw) == -2, kw
    for kw in unsupported:
        assert step(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(s._state, state0) and bool(torch.isnan(f0).all()) and bool(torch.isnan(vp).all()) and bool((st == -7).all())
    # a step whose n_seen is not the stream's launches, and changes nothing either
    assert step(n_seen=1920) == 0
    torch.cuda.synchronize()
    assert torch.equal(s._state, state0) and bool(torch.isnan(f0).all()) and bool((st == -7).all())
    # a valid call right after gives the op's bits
    twin = StreamF0(2, lag=4)
    twin._state.copy_(state0)
    twin._n_seen, twin._emitted = 2048, s.frames_out
    want = twin.push(x)
    assert step() == 0
    torch.cuda.synchronize()
    m = want[0].shape[1]
    assert m == 2 and torch.equal(f0[:, :m], want[0]) and torch.equal(vp[:, :m], want[1]) and torch.equal(st[:, :m], want[2])
    assert bool(torch.isnan(f0[:, m:]).all()) and torch.equal(s._state, twin._state)
    # the binding refuses what it can see, with a text
    b = engine.binding()
    outs = (torch.empty(2, 4, device="cuda"), torch.empty(2, 4, dtype=torch.float64, device="cuda"), torch.empty(2, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="lag"):
        b.pyin_stream_step(twin._state, table, *cfg, 300, x, 2304, False, False, 0.0, *outs)
    with pytest.raises(RuntimeError, match="table"):
        b.pyin_stream_step(twin._state, fe._table((16000.0, 100.0, 800.0, 1024, 128), a.device), *cfg, 4, x, 2304, False, False, 0.0, *outs)
    with pytest.raises(RuntimeError, match="state"):
        b.pyin_stream_step(twin._state[:-8], table, *cfg, 4, x, 2304, False, False, 0.0, *outs)
    with pytest.raises(RuntimeError, match="voiced_prob"):
        b.pyin_stream_step(twin._state, table, *cfg, 4, x, 2304, False, False, 0.0, outs[0], outs[0], outs[2])
    with pytest.raises(RuntimeError, match=">= 2"):
        b.pyin_stream_step(twin._state, table, *cfg, 4, x, 2304, False, False, 0.0, *[o[:, :1].contiguous() for o in outs])
    twin.check()


@pytest.mark.parametrize("n", [128, 256 * 128])
def test_the_step_that_computes_frame_zero_stays_inside_its_scratch(n):
    """from n_seen = W a step of n samples computes n // hop + 1 frames, one more than any later step of that size: the scratch of
    nws_pyin_stream_workspace_bytes holds them (a pattern behind it stays intact) and the frames are the offline ones"""
    from nws_amd import _lib
    from nws_amd.data.utils import f0_extraction as fe
    from nws_amd.streaming import StreamF0
    L = _lib.lib()
    c, a, whole, _ = _offline("long_5s")
    cfg = (c.sr, c.fmin, c.fmax, c.frame_length, c.hop)
    s = StreamF0(1, lag=0)
    s.push(a[:, :512])
    assert s.frames_out == 0
    need = L.nws_pyin_stream_workspace_bytes(1, n, *cfg, 0)
    ws = torch.full((need + 16384,), 0xA5, dtype=torch.uint8, device="cuda")
    m = n // 128 + 1
    outs = (torch.empty(1, m, device="cuda"), torch.empty(1, m, dtype=torch.float64, device="cuda"), torch.empty(1, m, dtype=torch.int32, device="cuda"))
    x = a[:, 512:512 + n].contiguous()
    rc = L.nws_pyin_stream_step(s._state.data_ptr(), s._state.numel(), x.data_ptr(), 1, n, 512, *cfg, 0, fe._table(cfg, a.device).data_ptr(), 0,
                                0, 0.0, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), m, ws.data_ptr(), need,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((ws[need:] == 0xA5).all())
    assert torch.equal(outs[1], whole[1][:, :m])           # voiced_prob of frames 0 .. n // hop, as offline
    s._n_seen, s._emitted = 512 + n, m
    s.check()


def test_timbre_transfer_with_a_lag_of_the_whole_clip_writes_the_same_wav(tmp_path):
    """the model draws its oscillators' start phases and its noise from torch's generators, which two processes seed differently:
    both runs fix them with the same --seed"""
    sr = 16000
    t = np.arange(sr // 2) / sr
    x = (0.3 * np.sin(2 * np.pi * 220.0 * t) * np.minimum(1.0, 10 * t)).astype(np.float32)
    src, plain, streamed = str(tmp_path / "in.wav"), str(tmp_path / "plain.wav"), str(tmp_path / "streamed.wav")
    wavfile.write(src, sr, x)
    script = os.path.join(ROOT, "scripts", "timbre_transfer.py")
    for dst, extra in ((plain, ["--seed", "3"]), (streamed, ["--seed", "3", "--stream-f0", "255", "--chunk", "300"])):
        r = subprocess.run([sys.executable, script, src, dst, "--use-fastnewt", *extra], capture_output=True, text=True, timeout=300,
                           cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(plain, "rb") as f, open(streamed, "rb") as g:
        want = f.read()
        assert len(want) > 4 * x.size                      # float32 samples of the input's length behind the header
        assert want == g.read()
