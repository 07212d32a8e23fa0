"""CPU tests of the fixed-lag pYIN stream: the lagged backtrace of tests/pyin_stream_restatement.py against
the offline restatement, the host arithmetic of the C ABI against brute force, the refusals that need no device, and the
agreement of a four-frame lag with the offline decode on the signals of tests/test_gpu_pyin.py."""
import ctypes as C
import functools
import importlib
import os
import re

import numpy as np
import pytest

import pyin_restatement as pr
import pyin_stream_restatement as ps
from conftest import ROOT
from test_gpu_pyin import _cases

PKG = "neural-waveshaping-synthesis_amd"
CONFIGS = ({}, {"frame_length": 256, "hop_length": 100})


def _lib():
    return importlib.import_module(PKG + "._lib").lib()


def _cfg(c):
    return (c.sr, c.fmin, c.fmax, c.frame_length, c.hop)


def signals():
    """the twelve signals of test_gpu_pyin._cases, long_10s cut to 4 s"""
    return {name: (x[:4 * 16000] if name == "long_10s" else x, kw) for name, (x, kw) in _cases().items()}


@functools.lru_cache(maxsize=None)
def decoded(name):
    """offline restatement (float64 from the float32 samples) + the forward pass's argmax and backpointers: once per signal"""
    x, kw = signals()[name]
    c = pr.config(**kw)
    r = pr.pyin(x.astype(np.float32).astype(np.float64), c)
    arg, back = ps.forward(r.cand_bin, r.cand_prob, r.count, r.voiced_prob, c)
    return c, r, arg, back


@pytest.mark.parametrize("name", list(signals()))
def test_a_lag_of_the_whole_clip_is_the_offline_decode(name):
    c, r, arg, back = decoded(name)
    T = len(arg)
    assert T == pr.n_frames(signals()[name][0].size, c)
    assert np.array_equal(ps.lagged(arg, back, T), r.states)
    assert np.array_equal(ps.lagged(arg, back, T - 1), r.states)
    # a stream that ended with fewer computed frames decodes its tail from the last frame all the same
    assert np.array_equal(ps.lagged(arg, back, 255 if T <= 256 else T, computed=max(1, T - 5)), r.states)


@pytest.mark.parametrize("name", list(signals()))
def test_lag_four_agrees_with_offline(name):
    c, r, arg, back = decoded(name)
    got = ps.lagged(arg, back, 4)
    v_off, v_lag = r.states < c.n_bins, got < c.n_bins
    both = v_off & v_lag
    flags = float(np.mean(v_off == v_lag))
    bins = float(np.mean(got[both] == r.states[both])) if both.any() else 1.0
    print(name, "frames", len(arg), "voiced flags equal", flags, "bins equal where both voiced", bins)
    assert np.array_equal(v_off, v_lag)
    assert np.array_equal(got[both], r.states[both])


def test_agreement_table_per_lag():
    """the table of the definition: the share of equal voiced flags, lowest and highest over the signals, per lag"""
    rows = {}
    for L in (0, 2, 3, 4, 8):
        flags, bins = [], []
        for name in signals():
            c, r, arg, back = decoded(name)
            got = ps.lagged(arg, back, L)
            v_off, v_lag = r.states < c.n_bins, got < c.n_bins
            both = v_off & v_lag
            flags.append(float(np.mean(v_off == v_lag)))
            bins.append(float(np.mean(got[both] == r.states[both])) if both.any() else 1.0)
        rows[L] = (min(flags), max(flags), min(bins))
        print("lag", L, "voiced flags equal: %.1f .. %.1f %%" % (100 * min(flags), 100 * max(flags)), "bins equal: %.1f %%" % (100 * min(bins)))
    # asserted: what the definition promises (lag 4 and above).  The shorter lags are printed for DESIGN.md 3.24: here lags 2
    # and 3 differ from offline on one frame of hop_64 (76 frames, a hop of 4 ms: three frames are 12 ms), lag 0 on up to 6 %.
    for L in (4, 8):
        assert rows[L] == (1.0, 1.0, 1.0), (L, rows[L])
    for L in (0, 2, 3):
        assert rows[L][2] == 1.0, (L, rows[L])            # a bin never differs where both decodes are voiced


def test_host_arithmetic_equals_brute_force():
    L = _lib()
    for kw in CONFIGS:
        c = pr.config(**kw)
        cfg = _cfg(c)
        assert L.nws_pyin_stream_max_chunk(*cfg) == ps.max_chunk(c) == 256 * c.hop
        for B in (1, 3, 65535):
            assert L.nws_pyin_stream_state_bytes(B, *cfg) == ps.state_bytes(B, c)
        for n in range(0, 3 * c.frame_length + 1):
            F = ps.frames_computed(n, c)
            assert L.nws_pyin_stream_frames(n, *cfg, 0) == F, (kw, n)
            T = ps.frames_total(n, c) if n > c.W else -1             # a stream that short cannot end
            assert L.nws_pyin_stream_frames(n, *cfg, 1) == T, (kw, n)
            for lag in (0, 1, 8):
                assert L.nws_pyin_stream_emitted(n, *cfg, lag, 0) == ps.frames_emitted(n, c, lag) == max(0, F - lag), (kw, n, lag)
                assert L.nws_pyin_stream_emitted(n, *cfg, lag, 1) == T, (kw, n, lag)
        # the scratch of a step holds the most frames one of its passes can compute, whatever the stream has seen: one more than
        # n // hop for the step that starts at n_seen = W and computes frame 0 with the rest
        for n in (1, c.hop - 1, c.hop, c.hop + 1, 2 * c.hop, 1000, 8 * c.hop, ps.max_chunk(c)):
            for final in (0, 1):
                frames = ps.max_new_frames(n, c, bool(final))
                assert frames >= (n // c.hop + 1 if not final else 1)
                for B in (1, 3):
                    assert L.nws_pyin_stream_workspace_bytes(B, n, *cfg, final) == ps.workspace_bytes(B, frames, c), (kw, n, final, frames)
        assert L.nws_pyin_stream_workspace_bytes(1, 0, *cfg, 1) == ps.workspace_bytes(1, ps.max_new_frames(0, c, True), c)
    cfg = _cfg(pr.config())
    assert L.nws_pyin_stream_frames(-1, *cfg, 0) == -1 and L.nws_pyin_stream_emitted(5, *cfg, 256, 0) == -1
    assert L.nws_pyin_stream_emitted(5, *cfg, -1, 0) == -1
    assert L.nws_pyin_stream_frames((1 << 21) * 128, *cfg, 0) >= 0 and L.nws_pyin_stream_frames((1 << 21) * 128 + 1, *cfg, 0) == -1
    # what nws_pyin_dims refuses, B outside 1 .. 65 535, more than 256 hops in half a frame
    bad = (16000.0, 65.0, 2093.0, 4096, 128)
    assert L.nws_pyin_stream_state_bytes(1, *bad) == 0 and L.nws_pyin_stream_max_chunk(*bad) == 0
    assert L.nws_pyin_stream_frames(5, *bad, 0) == -1 and L.nws_pyin_stream_emitted(5, *bad, 0, 0) == -1
    assert L.nws_pyin_stream_state_bytes(0, *cfg) == 0 and L.nws_pyin_stream_state_bytes(65536, *cfg) == 0
    dims = (C.c_int32 * 8)()
    fine = (16000.0, 65.0, 2093.0, 1024, 1)
    assert L.nws_pyin_dims(*fine, dims) == 0 and L.nws_pyin_stream_state_bytes(1, *fine) == 0     # 512 hops in half a frame
    assert L.nws_pyin_stream_state_bytes(1, 16000.0, 65.0, 2093.0, 1024, 2) > 0
    assert L.nws_pyin_stream_workspace_bytes(1, 128, *cfg, 0) > 0 and L.nws_pyin_stream_workspace_bytes(1, 256 * 128 + 1, *cfg, 0) == 0


def test_refusals_of_reset_and_step_come_before_any_launch():
    """no GPU here: a call that got as far as the runtime would return a HIP error code (positive), never -1 / -2"""
    L = _lib()
    c = pr.config()
    cfg = _cfg(c)
    need = L.nws_pyin_stream_state_bytes(2, *cfg)
    buf = np.zeros(need // 4 + (1 << 16), dtype=np.float32)
    p, nbytes = buf.ctypes.data, buf.nbytes
    ws_need = L.nws_pyin_stream_workspace_bytes(2, 256, *cfg, 0)
    assert L.nws_pyin_stream_reset(None, nbytes, 2, *cfg, None) == -2
    assert L.nws_pyin_stream_reset(p, nbytes, 0, *cfg, None) == -2
    assert L.nws_pyin_stream_reset(p, need - 1, 2, *cfg, None) == -2
    assert L.nws_pyin_stream_reset(p, nbytes, 65536, *cfg, None) == -1
    assert L.nws_pyin_stream_reset(p, nbytes, 2, 16000.0, 65.0, 2093.0, 4096, 128, None) == -1

    def step(state=p, size=nbytes, x=p, B=2, n=256, n_seen=2048, cfg=cfg, lag=4, table=p, final=0, f0=p, vp=p, states=p, stride=2,
             ws=p, ws_bytes=1 << 40):
        return L.nws_pyin_stream_step(state, size, x, B, n, n_seen, *cfg, lag, table, final, 0, 0.0, f0, vp, states, stride, ws,
                                      ws_bytes, None)

    assert step(state=None) == -2 and step(table=None) == -2 and step(f0=None) == -2 and step(vp=None) == -2
    assert step(states=None) == -2 and step(ws=None) == -2 and step(x=None) == -2
    assert step(B=0) == -2 and step(n=-1) == -2 and step(n_seen=-1) == -2
    assert step(n=0) == -2                                              # an empty chunk that is not final
    assert step(n=12, n_seen=500, final=1) == -2                        # N = 512 = frame_length / 2: the stream cannot end
    assert step(n=0, n_seen=512, final=1) == -2
    assert step(stride=1) == -2                                         # 256 samples after 2048 at lag 4: frames 9 and 10 leave
    assert step(n=0, final=1, n_seen=2048, stride=7) == -2              # a flush at lag 4: frames 9 .. 16, eight of them
    assert step(n=256, final=1, n_seen=2048, stride=9) == -2            # 2 + the flush's 8
    assert step(size=need - 1) == -2 and step(ws_bytes=ws_need - 1) == -2
    assert step(lag=-1) == -2 and step(lag=256) == -2
    assert step(n=256 * 128 + 1, stride=1000) == -1
    assert step(B=65536) == -1 and step(cfg=(16000.0, 65.0, 2093.0, 4096, 128)) == -1 and step(cfg=(16000.0, 65.0, 2093.0, 1024, 1)) == -1
    assert step(n_seen=(1 << 21) * 128) == -1
    assert not buf.any()                                                # nothing wrote the host buffer either


def test_header_abi_build_sources_and_shared_code():
    with open(os.path.join(ROOT, "include", "nws_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define NWS_ABI_VERSION 6\b", header)
    for name in ("state_bytes", "max_chunk", "workspace_bytes", "reset", "frames", "emitted", "step"):
        assert re.search(r"\bnws_pyin_stream_" + name + r"\(", header), name
    build = importlib.import_module(PKG + ".build")
    assert "pyin_stream.hip" in build.SOURCES and "pyin.hip" in build.SOURCES
    assert "-fno-slp-vectorize" in build.EXTRA_FLAGS["pyin_stream.hip"]
    # the per-frame work exists once: both forms include the header, neither defines the shared functions itself
    shared = ("sqdiff_sum", "pyin_cmnd_tile", "pyin_observe_block", "pyin_maxplus", "pyin_wave_max", "pyin_global_max", "pyin_predecessor")
    with open(os.path.join(build.CSRC, "pyin_frame.h")) as f:
        frame = f.read()
    for fn in shared:
        assert len(re.findall(r"__device__ __forceinline__ \w+ " + fn + r"\(", frame)) == 1, fn
    for src in ("pyin.hip", "pyin_stream.hip"):
        with open(os.path.join(build.CSRC, src)) as f:
            text = f.read()
        assert '#include "pyin_frame.h"' in text
        for fn in shared:
            assert not re.search(r"__device__[^;{]*\b" + fn + r"\(", text), (src, fn)
        assert sum(text.count(fn + "(") + text.count(fn + "<") for fn in shared) >= 4, src


def test_stream_f0_raises_without_a_device():
    streaming = importlib.import_module(PKG + ".streaming")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        streaming.StreamF0(1, device="cpu")
