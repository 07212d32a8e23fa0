"""CPU tests of the releasing loudness reference: the restatement of tests/loudness_release_restatement.py push
by push against its closed form and, at rho = 1, against tests/loudness_stream_restatement.py; the closed form of the level
(consequence 6), the recovery after a click (consequence 7), the flush rule, the release factor, the refusals of the new entry
points that need no device, the surface of both bindings, the scripts' option and the packaged gin file."""
import ctypes as C
import importlib
import importlib.util
import os
import re

import numpy as np
import pytest

import loudness_release_restatement as lr
import loudness_stream_restatement as ls
from conftest import ROOT
from test_cpu_loudness_stream import _chunkings, analysed

PKG = "neural-waveshaping-synthesis_amd"

# (n_fft, hop, N), release in dB/s at 16 kHz (0.5, 0.5, 0.25 dB per frame), the frame equality is asserted from
RECOVERY = (((256, 100, 30001), 80.0, 80), ((1024, 128, 40000), 62.5, 70), ((64, 16, 9000), 250.0, 170))


def _lib():
    return importlib.import_module(PKG + "._lib").lib()


def _rho(db_per_frame):
    return lr.release_factor(db_per_frame * 16000.0, 1, 16000.0)


@pytest.mark.parametrize("name", ["noise_short_odd_length", "small_fft_hop_not_pow2", "silence_then_click"])
def test_push_by_push_equals_the_closed_form_whatever_the_chunking(name):
    x, n_fft, hop, P, _ = analysed(name)
    for rho in (_rho(0.05), _rho(3.0)):
        for kw in (dict(), dict(floor=0.01 * P.max())):
            for L in (0, 4, 8):
                closed, closed_ref = lr.stream_of_power(P, x.size, n_fft, hop, L, rho, **kw)
                runs = {tag: lr.run_chunks(x, chunks, n_fft, hop, L, rho=rho, **kw) for tag, chunks in _chunkings(x.size, hop).items()}
                for tag, (loud, ref, counts) in runs.items():
                    assert np.array_equal(loud, runs["whole"][0]) and np.array_equal(ref, runs["whole"][1]), (name, L, tag)
                    # the frames computed as the samples arrive are the whole clip's (another FFT call: not bit for bit)
                    assert np.abs(loud - closed).max() <= 1e-12 and np.allclose(ref, closed_ref, rtol=1e-12, atol=1e-300), (name, L, tag)
                    assert sum(counts) == len(closed)
                assert runs["hops"][2] == ls.run_chunks(x, _chunkings(x.size, hop)["hops"], n_fft, hop, L)[2]     # emission is 3.25's


@pytest.mark.parametrize("name", ["noise_short_odd_length", "small_fft_hop_not_pow2", "silence_then_click", "all_zero"])
def test_without_a_release_both_forms_are_the_running_stream_exactly(name):
    x, n_fft, hop, P, _ = analysed(name)
    for kw, kw0 in ((dict(), dict()), (dict(floor=0.5 * P.max()), dict(initial=0.5 * P.max())),
                    (dict(track=False, floor=0.37 * P.max()), dict(track=False, initial=0.37 * P.max()))):
        for L in (0, 4, 255):
            want = ls.stream_of_power(P, x.size, n_fft, hop, L, **kw0)
            got = lr.stream_of_power(P, x.size, n_fft, hop, L, 1.0, **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, kw, L)
        chunks = _chunkings(x.size, hop)["irregular"]
        want, got = ls.run_chunks(x, chunks, n_fft, hop, 4, **kw0), lr.run_chunks(x, chunks, n_fft, hop, 4, rho=1.0, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_the_level_is_the_maximum_of_every_frames_own_decaying_term():
    """consequence 6 on 200 frames in np.float32: rounding and the flush are monotone, so g commutes with max"""
    g = np.random.default_rng(11)
    p = (g.uniform(0, 1, 200) ** 8 * np.where(g.uniform(size=200) < 0.1, 1e3, 1.0)).astype(np.float32)
    p[50:60] = 0.0
    for rho in (_rho(0.05), _rho(0.5), _rho(3.0), _rho(40.0)):
        for floor in (0.0, 1e-3):
            M = lr.levels(p, rho, floor, dtype=np.float32)
            assert M.dtype == np.float32 and np.array_equal(M, lr.levels_closed_form(p, rho, floor)), (rho, floor)
            assert np.all(M >= p) and np.all(M >= np.float32(floor))
    assert np.array_equal(lr.levels(p, 1.0, 0.0, dtype=np.float32), np.maximum.accumulate(p))


@pytest.mark.parametrize("config, release, first_equal", RECOVERY)
def test_the_reference_recovers_after_a_click(config, release, first_equal):
    """consequence 7: from the frame on at which the click's decayed term lies below the other terms, the stream on the clip
    with the click equals the stream on the clip without it - reference and loudness, exactly"""
    n_fft, hop, N = config
    x, clean = lr.recovery_input(n_fft, hop, N)
    rho = lr.release_factor(release, hop, 16000)
    assert abs(-10 * np.log10(rho) - (0.25 if hop == 16 else 0.5)) < 1e-6
    P, Pc = ls.lo.stft_magnitude(x, n_fft, hop) ** 2, ls.lo.stft_magnitude(clean, n_fft, hop) ** 2
    T = P.shape[1]
    for L in (0, 8):
        (loud, ref), (loud_c, ref_c) = lr.stream_of_power(P, N, n_fft, hop, L, rho), lr.stream_of_power(Pc, N, n_fft, hop, L, rho)
        differ = np.nonzero((ref != ref_c) | (loud != loud_c))[0]
        print(config, "lag", L, "last differing frame", differ.max(), "of", T)
        assert differ.max() < first_equal and T - 1 - differ.max() >= 200
        assert np.array_equal(ref[first_equal:], ref_c[first_equal:]) and np.array_equal(loud[first_equal:], loud_c[first_equal:])
        # the same in the fp32 recurrence the kernels run
        M32, M32c = (lr.window_refs(lr.levels(q.max(axis=0).astype(np.float32), rho, dtype=np.float32), N, n_fft, hop, L) for q in (P, Pc))
        assert np.nonzero(M32 != M32c)[0].max() < first_equal and np.array_equal(M32[first_equal:], M32c[first_equal:])
        # without a release the click pins the reference: more than 90 % of the frames differ
        pinned, pinned_c = ls.stream_of_power(P, N, n_fft, hop, L)[1], ls.stream_of_power(Pc, N, n_fft, hop, L)[1]
        assert np.mean(pinned != pinned_c) > 0.9


def test_a_frames_reference_is_never_below_its_own_peak():
    for name in ("noise_short_odd_length", "silence_then_click", "decrescendo"):
        x, n_fft, hop, P, _ = analysed(name)
        for rho in (_rho(0.05), _rho(3.0), _rho(40.0)):
            for L in (0, 4, 255):
                loud, ref = lr.stream_of_power(P, x.size, n_fft, hop, L, rho)
                assert np.all(ref >= P.max(axis=0)) and loud.max() <= 1.0 + 1e-12, (name, rho, L)
    # the window is what makes it so: the level at e + L alone can lie below p(e)
    x, n_fft, hop, P, _ = analysed("decrescendo")
    M = lr.levels(P.max(axis=0), _rho(40.0))
    assert np.any(M[8:] < P.max(axis=0)[:-8])


def test_a_decayed_level_is_flushed_to_the_floor():
    """once rho M falls below 2^-126 the level is exactly F, in either dtype and whatever the denormal mode"""
    rho = _rho(40.0)                                             # 1e-4 per frame
    p = np.zeros(40, dtype=np.float32)
    p[0] = 1.0
    for dtype in (np.float32, np.float64):
        for floor in (0.0, 1e-30):
            M = lr.levels(p, rho, floor, dtype=dtype)
            gone = int(np.nonzero(M == dtype(floor))[0][0])
            assert 1 <= gone <= 11 and np.all(M[gone:] == dtype(floor)) and np.all(np.diff(M[:gone + 1]) < 0), (dtype, floor, M[:12])
    M = lr.levels(p, rho, 0.0, dtype=np.float32)
    assert M[9] > 0 and M[9] * np.float32(rho) < lr.TINY and M[10] == 0.0        # no denormal level is ever stored
    assert lr.decay(np.float32(2.0 ** -120), 0.5, np.float32) == np.float32(2.0 ** -121) and lr.decay(np.float32(2.0 ** -126), 0.5, np.float32) == 0.0


def test_release_factor_is_rounded_once_from_float64():
    le = importlib.import_module(PKG + ".data.utils.loudness_extraction")
    for hop, sr in ((128, 16000), (16, 16000)):
        for rate in (0.0, 3.0, 6.0, 12.0, 62.5, 250.0):
            want = float(np.float32(10.0 ** (-rate * hop / (10.0 * sr))))
            got = le.release_factor(rate, hop, sr)
            assert got == want == lr.release_factor(rate, hop, sr) and isinstance(got, float) and 0.0 < got <= 1.0
            assert abs(got - 10.0 ** (-rate * hop / (10.0 * sr))) <= 2.0 ** -24
        assert le.release_factor(0.0, hop, sr) == 1.0 and le.release_factor(1e-9, hop, sr) == 1.0      # rounds to no release
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            le.release_factor(bad, 128, 16000)
    with pytest.raises(RuntimeError):
        le.release_factor(1e9, 128, 16000)                        # the factor underflows to 0


def test_blob_sizes():
    """a stream without a release keeps the blob of 3.25; a releasing one appends float F[B], padded to 8 bytes"""
    L = _lib()
    for n_fft, hop in ((1024, 128), (256, 100), (64, 16)):
        for B in (1, 2, 3, 65535):
            base = L.nws_loudness_stream_state_bytes(B, n_fft, hop)
            assert base == ls.state_bytes(B, n_fft)
            assert L.nws_loudness_stream_release_state_bytes(B, n_fft, hop) == base + (4 * B + 7) // 8 * 8
    for n_fft, hop in ((1000, 128), (4096, 128), (1024, 1), (1024, 0)):
        assert L.nws_loudness_stream_release_state_bytes(1, n_fft, hop) == 0
    assert L.nws_loudness_stream_release_state_bytes(0, 1024, 128) == 0 and L.nws_loudness_stream_release_state_bytes(65536, 1024, 128) == 0
    # the whole-clip extractor: the offline workspace and M (B, T), padded to 256
    for B, N in ((1, 4099), (3, 64000)):
        T = 1 + N // 128
        assert L.nws_loudness_causal_workspace_bytes(B, N, 1024, 128) == L.nws_loudness_workspace_bytes(B, N, 1024, 128) + (4 * B * T + 255) // 256 * 256
    assert L.nws_loudness_causal_workspace_bytes(1, 4099, 1024, 1) == 0 and L.nws_loudness_workspace_bytes(1, 4099, 1024, 1) > 0
    assert L.nws_loudness_causal_workspace_bytes(0, 4099, 1024, 128) == 0 and L.nws_loudness_causal_workspace_bytes(1, 4099, 4096, 128) == 0
    assert L.nws_loudness_causal_workspace_bytes(1, (1 << 21) * 16 + 1, 64, 16) == 0


def test_refusals_of_the_new_entry_points_come_before_any_launch():
    """no GPU here: a call that got as far as the runtime would return a HIP error code (positive), never -1 / -2 / -3"""
    L = _lib()
    need = L.nws_loudness_stream_release_state_bytes(2, 1024, 128)
    base = L.nws_loudness_stream_state_bytes(2, 1024, 128)
    buf = np.zeros(need // 4 + (1 << 16), dtype=np.float32)
    p, nbytes = buf.ctypes.data, buf.nbytes
    assert L.nws_loudness_stream_reset_release(None, nbytes, 2, 1024, 128, p, None) == -2
    assert L.nws_loudness_stream_reset_release(p, nbytes, 2, 1024, 128, None, None) == -2
    assert L.nws_loudness_stream_reset_release(p, nbytes, 0, 1024, 128, p, None) == -2
    assert L.nws_loudness_stream_reset_release(p, need - 1, 2, 1024, 128, p, None) == -2
    assert L.nws_loudness_stream_reset_release(p, base, 2, 1024, 128, p, None) == -2          # the blob of a stream without a release
    assert L.nws_loudness_stream_reset_release(p, nbytes, 65536, 1024, 128, p, None) == -1
    assert L.nws_loudness_stream_reset_release(p, nbytes, 2, 1024, 1, p, None) == -1

    def step(state=p, size=nbytes, x=p, B=2, n=256, n_seen=2048, n_fft=1024, hop=128, lag=4, rho=0.9, track=1, dft=p, amin=1e-5,
             top_db=80.0, final=0, loud=p, ref=p, stride=2, ws=p, ws_bytes=1 << 40):
        return L.nws_loudness_stream_step_release(state, size, x, B, n, n_seen, n_fft, hop, lag, rho, track, dft, amin, top_db, 1, final,
                                                  loud, ref, stride, ws, ws_bytes, None)

    for rho in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert step(rho=rho) == -2, rho
        assert step(rho=rho, track=0) == -2, rho
    assert step(rho=0.5, track=0) == -2 and step(rho=float(np.nextafter(np.float32(1), np.float32(0))), track=0) == -2
    assert step(size=need - 1) == -2 and step(size=base) == -2                                 # rho < 1 needs the floors
    assert step(rho=1.0, size=base - 1) == -2
    # and everything nws_loudness_stream_step refuses
    assert step(state=None) == -2 and step(dft=None) == -2 and step(loud=None) == -2 and step(ref=None) == -2
    assert step(ws=None) == -2 and step(x=None) == -2 and step(B=0) == -2 and step(n=-1) == -2 and step(n_seen=-1) == -2
    assert step(n=0) == -2 and step(n=12, n_seen=500, final=1) == -2 and step(stride=1) == -2
    assert step(lag=-1) == -2 and step(lag=256) == -2 and step(amin=0.0) == -2 and step(top_db=-1.0) == -2
    assert step(ws_bytes=L.nws_loudness_stream_workspace_bytes(2, 256, 1024, 128, 0) - 1) == -2
    assert step(n=256 * 128 + 1, stride=1000) == -1 and step(B=65536) == -1 and step(n_fft=4096) == -1 and step(hop=1) == -1
    assert step(n_seen=(1 << 21) * 128) == -1

    def causal(audio=p, B=2, N=4099, n_fft=1024, hop=128, dft=p, lag=8, rho=0.9, floor=p, track=1, amin=1e-5, top_db=80.0, loud=p,
               ref=p, peak=p, ws=p, ws_bytes=1 << 40):
        return L.nws_loudness_causal(audio, B, N, n_fft, hop, dft, lag, rho, floor, track, amin, top_db, 1, loud, ref, peak, ws, ws_bytes,
                                     None)

    # nws_loudness's refusals
    assert causal(audio=None) == -2 and causal(dft=None) == -2 and causal(loud=None) == -2 and causal(ws=None) == -2 and causal(B=0) == -2
    assert causal(N=512) == -2 and causal(n_fft=1000) == -2 and causal(hop=1025) == -2 and causal(amin=0.0) == -2 and causal(top_db=-1.0) == -2
    assert causal(B=65536) == -1
    assert causal(ws_bytes=L.nws_loudness_causal_workspace_bytes(2, 4099, 1024, 128) - 1) == -3
    # its own
    assert causal(ref=None) == -2 and causal(peak=None) == -2 and causal(lag=-1) == -2 and causal(lag=256) == -2
    for rho in (0.0, -1.0, 1.5, float("nan")):
        assert causal(rho=rho) == -2
    assert causal(rho=0.5, track=0) == -2 and causal(rho=1.0, track=0, floor=None) == -2
    # a configuration the stream refuses: more than 256 hops in half a frame
    assert causal(hop=1) == -1 and L.nws_loudness_workspace_bytes(2, 4099, 1024, 1) > 0
    assert not buf.any()                                                # nothing wrote the host buffer either


def test_new_symbols_in_the_header_and_both_bindings():
    with open(os.path.join(ROOT, "include", "nws_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define NWS_ABI_VERSION 6\b", header)
    lib_mod = importlib.import_module(PKG + "._lib")
    L = lib_mod.lib()
    for name in ("nws_loudness_stream_release_state_bytes", "nws_loudness_stream_reset_release", "nws_loudness_stream_step_release",
                 "nws_loudness_causal_workspace_bytes", "nws_loudness_causal"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    with open(os.path.join(ROOT, PKG, "csrc", "torch_ops.cpp")) as f:
        ops = f.read()
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    for op in ("loudness_stream_reset_release", "loudness_stream_step_release", "loudness_causal"):
        assert re.search(r'm\.def\("' + op + r"\(", ops) and callable(getattr(cops, op)), op
    # the refusals carry the same texts in both
    with open(os.path.join(ROOT, PKG, "_cops.py")) as f:
        ctext = f.read()
    for text in ("release_factor ", " outside (0, 1]", ": a release needs a tracked reference", "loudness_causal: lag "):
        assert text in ops and text in ctext, text
    build = importlib.import_module(PKG + ".build")
    assert "loudness_causal.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["loudness_causal.hip"]
    # one level recurrence and one dB pass for the stream and the extractor
    for src in ("loudness_stream.hip", "loudness_causal.hip"):
        with open(os.path.join(build.CSRC, src)) as f:
            text = f.read()
        assert '#include "loudness_level.h"' in text and '#include "loudness_db.h"' in text and text.count("loudness_level_step(") == 1
        assert text.count("loudness_frame_db(") == 1 and "__fmul_rn" not in text, src


def test_stream_loudness_and_the_extractor_raise_without_a_device():
    streaming = importlib.import_module(PKG + ".streaming")
    le = importlib.import_module(PKG + ".data.utils.loudness_extraction")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        streaming.StreamLoudness(1, device="cpu", release_db_per_s=6.0)
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        le.causal_loudness_frames(torch.zeros(1, 4000), 1024, 128)


def _script_module(name):
    spec = importlib.util.spec_from_file_location("script_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_scripts_have_the_release_option_and_it_is_off_by_default():
    for name, opt in (("live_transfer", "loudness_release"), ("timbre_transfer", "loudness_release"), ("time_control_stream", "release")):
        params = {p.name: p for p in _script_module(name).main.params}
        assert opt in params and params[opt].default == 0.0 and "--" + opt.replace("_", "-") in params[opt].opts, name
    import inspect
    streaming = importlib.import_module(PKG + ".streaming")
    for cls in (streaming.StreamLoudness, streaming.StreamControl):
        assert inspect.signature(cls.__init__).parameters["release_db_per_s"].default == 0.0
    assert inspect.signature(streaming.StreamLoudness.__init__).parameters["sample_rate"].default == 16000


def test_the_live_gin_file_binds_the_causal_extractor():
    nws = importlib.import_module(PKG)
    le = importlib.import_module(PKG + ".data.utils.loudness_extraction")
    gin = nws.gin
    saved = {k: dict(v) for k, v in gin._BINDINGS.items()}, dict(gin._MACROS)
    try:
        gin.parse_config_file(os.path.join(ROOT, PKG, "gin", "data", "urmp_4second_pyin_live.gin"))
        assert gin.query_parameter("preprocess_audio.loudness_extractor") is le.extract_causal_loudness
        assert gin.query_parameter("extract_causal_loudness.lag") == 8 and gin.query_parameter("extract_causal_loudness.n_fft") == 1024
        assert gin.query_parameter("extract_causal_loudness.hop_length") == 128
        assert gin.query_parameter("extract_causal_loudness.release_db_per_s") == 0.0
        assert gin.query_parameter("extract_causal_loudness.interpolate_fn") is None
        assert gin.query_parameter("extract_f0_with_pyin.hop_length") == 128              # the file it includes
    finally:
        gin._BINDINGS.clear()
        gin._BINDINGS.update(saved[0])
        gin._MACROS.clear()
        gin._MACROS.update(saved[1])
    import inspect
    sig, base = inspect.signature(le.extract_causal_loudness), inspect.signature(le.extract_perceptual_loudness)
    assert list(sig.parameters)[:8] == list(base.parameters) and list(sig.parameters)[8:] == ["lag", "release_db_per_s", "floor_power"]
    assert all(sig.parameters[k].default == base.parameters[k].default for k in list(base.parameters)[1:])
