"""-m gpu: stateful streaming on the runtime-size path (csrc/generic.hip nws_g_stream_step) - `model.stream(B)` on
a model `Engine.specialised()` turns down.  Anchor, as for the packaged stream (tests/test_gpu_streaming.py): the concatenation of
the streamed chunks equals the oracle's ONE-SHOT forward up to the reverb input for any chunking, and the reverb is a linear
convolution of the stream.  Two size sets (tests/g_stream_models.py), each with exact shapers and as FastNEWT."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
from scipy.signal import fftconvolve

from conftest import rms
from g_stream_models import BANK_GIN, build, build_from_gin, inputs, oracle_for, run_stream
from gpu_util import maxabs, record

pytestmark = pytest.mark.gpu

BAD_ARG, WORKSPACE = -2, -3     # include/nws_hip.h
PKG = "neural-waveshaping-synthesis_amd"


@pytest.fixture(scope="module")
def models():
    """(sizes, fast) -> (model, state dict): built once, shared, never edited (tests that edit weights copy)"""
    cache = {}

    def get(sizes, fast):
        if (sizes, fast) not in cache:
            cache[(sizes, fast)] = build(sizes, fast)
            assert not cache[(sizes, fast)][0]._engine.specialised()
        return cache[(sizes, fast)]

    return get


_REFS = {}


def reference(models, sizes, fast, B, F):
    """one oracle run per (sizes, fast, B, F), shared by the schedules: inputs, pre_ref, y_ref, tail_ref, the yardstick"""
    key = (sizes, fast, B, F)
    if key not in _REFS:
        model, w = models(sizes, fast)
        f0, control, pu, nz = inputs(sizes, B, F, F * 7 + B)
        st = {}
        oracle_for(sizes, w, fast)(f0, control, pu, nz, stages=st)
        pre_ref = st["pre_reverb"].numpy()
        ir_ = np.concatenate([[0.0], w["reverb.ir"].reshape(-1).astype(np.float64)])
        full = np.stack([fftconvolve(pre_ref[b].astype(np.float64), ir_) for b in range(B)])
        with torch.no_grad():
            own = model.pre_reverb(f0.cuda(), control.cuda(), phase_u=pu.cuda(), noise=nz.cuda()).cpu().numpy().reshape(B, -1)
        _REFS[key] = dict(f0=f0, control=control, pu=pu, nz=nz, pre_ref=pre_ref, y_ref=pre_ref + full[:, :128 * F],
                          tail_ref=full[:, 128 * F:], yardstick=maxabs(own, pre_ref))
    return _REFS[key]


SCHEDULES = [([60], 3), ([1, 7, 16, 4, 31, 1], 3), ([2] * 30, 3)]


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("sizes,chunks,B", [("bank", c, b) for c, b in SCHEDULES] + [("bank", [1, 7, 16, 4, 31, 1], 17)]
                         + [("odd", c, b) for c, b in SCHEDULES])
def test_stream_equals_one_shot(models, sizes, chunks, B, fast):
    """The schedules of the packaged stream's test: a one-frame first chunk, a 31-frame chunk past the 2048-sample reverb switch,
    thirty steady two-frame hops (the captured hop runs), 17 rows (the batched noise kernel).  Bars: the packaged stream's.  The
    yardstick is the distance of the model's own one-shot pre_reverb from the same oracle signal; where a random-init model is
    loud enough for the yardstick itself to exceed the first bar, the bar is 4 x the yardstick (a stream sums the same products
    in at most a few other orders)."""
    model, _ = models(sizes, fast)
    F = sum(chunks)
    R = reference(models, sizes, fast, B, F)
    s, y, pre = run_stream(model, chunks, R["f0"], R["control"], R["pu"], R["nz"])
    assert pre.shape == (B, 128 * F) and y.shape == (B, 128 * F) and s.samples_emitted == 128 * F
    assert s.frames_seen == F and s.finished
    if chunks == [2] * 30:
        assert s._graphs, "the steady-state hop was never captured"
    e_pre = maxabs(pre, R["pre_ref"])
    e_y = rms(y - R["y_ref"])
    tail = s.reverb_tail().cpu().numpy()
    assert tail.shape == (B, s.tail_len)
    e_tail = rms(tail[:, :R["tail_ref"].shape[1]] - R["tail_ref"])
    pre_max = float(np.abs(R["pre_ref"]).max())
    bar = 2e-6 * max(1.0, pre_max / 1e-2)
    if R["yardstick"] > bar:
        bar = 4.0 * R["yardstick"]
    print(sizes, fast, chunks, B, dict(e_pre=e_pre, yardstick=R["yardstick"], bar=bar, pre_max=pre_max, e_y=e_y, y_rms=rms(R["y_ref"]),
                                       e_tail=e_tail))
    record(f"g_stream_{sizes}_{'fast' if fast else 'exact'}_chunks_{len(chunks)}x_B{B}", pre_max_abs_err=e_pre,
           one_shot_pre_max_abs_err=R["yardstick"], pre_bar=bar, pre_max=pre_max, y_rms_err=e_y, y_rms=rms(R["y_ref"]),
           tail_rms_err=e_tail, tail_rms=rms(R["tail_ref"]))
    assert e_pre <= bar
    assert e_y <= 1e-4 * max(1.0, rms(R["y_ref"])) and e_tail <= 1e-4 * max(1.0, rms(R["y_ref"]))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("sizes", ["bank", "odd"])
def test_chunking_invariance(models, sizes, fast):
    """The same 48 frames as one chunk, sixteen three-frame hops and [5, 43]: 1e-5 of the RMS, the bar DESIGN.md 3.8 states for a
    change of chunk size."""
    model, _ = models(sizes, fast)
    f0, control, pu, nz = inputs(sizes, 2, 48, 48)
    outs = [run_stream(model, chunks, f0, control, pu, nz) for chunks in ([48], [3] * 16, [5, 43])]
    y0, p0 = outs[0][1], outs[0][2]
    assert np.isfinite(y0).all() and rms(y0) > 1e-5
    for _, y, p in outs[1:]:
        print(sizes, fast, rms(y - y0) / rms(y0), rms(p - p0) / rms(p0))
        assert rms(y - y0) <= 1e-5 * rms(y0) and rms(p - p0) <= 1e-5 * rms(p0)


@pytest.mark.parametrize("sizes,fast", [("bank", False), ("odd", True)])
def test_graph_equals_eager(models, sizes, fast):
    """graph=True and graph=False streams on twelve two-frame hops give equal bits; static_io(2) / hop(2) continue the same stream
    with equal bits."""
    model, _ = models(sizes, fast)
    B, K, n = 2, 2, 15
    f0, control, pu, nz = inputs(sizes, B, K * n + 2, 9)
    chunks = [(f0[:, :, i * K:(i + 1) * K].cuda(), control[:, :, i * K:(i + 1) * K].cuda()) for i in range(n)]
    eager = model.stream(B, phase_u=pu.cuda(), noise=nz.cuda(), graph=False)
    s = model.stream(B, phase_u=pu.cuda(), noise=nz.cuda(), graph=True)
    for i, (a, c) in enumerate(chunks[:12]):
        assert torch.equal(s.push(a, c), eager.push(a, c)), i
    assert s._graphs and not eager._graphs
    for i, (a, c) in enumerate(chunks[12:]):
        f0_in, c_in, out = s.static_io(K)
        f0_in.copy_(a[:, 0])
        c_in.copy_(c)
        got = s.hop(K)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, eager.push(a, c)), i
        assert torch.equal(s._last_pre, eager._last_pre)
    assert s.samples_emitted == eager.samples_emitted == 128 * K * n - 64 and s.frames_seen == K * n


def test_weight_update_and_refresh(models):
    """After an in-place edit of newt.mixer.0.bias and refresh(), the captured stream and an eager one stay equal to the bit on the
    next four hops, and differ from the hops of an unedited twin."""
    model = copy.deepcopy(models("bank", False)[0])
    twin = copy.deepcopy(model)
    B, K = 1, 2
    f0, control, pu, nz = inputs("bank", B, 24, 5)
    hops = [(f0[:, :, i * K:(i + 1) * K].cuda(), control[:, :, i * K:(i + 1) * K].cuda()) for i in range(10)]
    a = model.stream(B, phase_u=pu.cuda(), noise=nz.cuda(), graph=True)
    b = model.stream(B, phase_u=pu.cuda(), noise=nz.cuda(), graph=False)
    t = twin.stream(B, phase_u=pu.cuda(), noise=nz.cuda(), graph=False)
    for x, c in hops[:6]:
        ya, yb, yt = a.push(x, c), b.push(x, c), t.push(x, c)
    assert a._graphs and torch.equal(ya, yb) and torch.equal(ya, yt)
    with torch.no_grad():
        model.newt.mixer[0].bias.add_(0.05)                # in place: nobody tells the engine
    a.refresh()
    b.refresh()
    assert not a._graphs                                   # dropped: they point into the old descriptor's tables
    for x, c in hops[6:]:
        ya, yb, yt = a.push(x, c), b.push(x, c), t.push(x, c)
        assert torch.equal(ya, yb) and not torch.equal(ya, yt)
    assert a._graphs                                       # captured again on the new record


def test_self_drawn_noise_and_long_chunks(models):
    """Without noise= every push draws nws_stream_noise_draws(...) values from the device generator: two streams after the same
    seed agree to the bit, and the output is finite.  A 300-frame push is split internally (249 + 51) and equals the same frames
    pushed as [150, 150] to the bar of test_chunking_invariance - compared on an injected noise vector: the device generator
    does not return the same values when one sequence is drawn in other pieces, so two chunkings of a self-drawn stream share
    the oscillator branch only (tests/test_gpu_streaming.py compares levels for that reason)."""
    _lib = importlib.import_module(PKG + "._lib")
    model, _ = models("bank", True)
    B, F = 2, 300
    f0, control, pu, nz = inputs("bank", B, F, 3)
    f0c, cc = f0.cuda(), control.cuda()
    drawn = []
    for _ in range(2):
        torch.manual_seed(3)
        s = model.stream(B, phase_u=pu.cuda())
        assert s._noise_all is None and s.max_frames == 249
        drawn.append(torch.cat([s.push(f0c[:, :, :40], cc[:, :, :40]), s.push(f0c[:, :, 40:], cc[:, :, 40:], final=True)], 1))
        assert s.samples_emitted == 128 * F and s.finished
    assert int(_lib.lib().nws_stream_noise_draws(40, 1, 0)) == 128 * 40 + 1
    assert drawn[0].shape == (B, 128 * F) and torch.isfinite(drawn[0]).all() and torch.equal(drawn[0], drawn[1])
    _, y_one, _ = run_stream(model, [300], f0, control, pu, nz)         # (the pre-reverb tap is the last piece's only)
    _, y_two, _ = run_stream(model, [150, 150], f0, control, pu, nz)
    assert y_one.shape == (B, 128 * F) and y_two.shape == (B, 128 * F)
    print(rms(y_one - y_two) / rms(y_one))
    assert rms(y_one - y_two) <= 1e-5 * rms(y_one)
    with pytest.raises(RuntimeError):
        s.push(f0c[:, :, :4], cc[:, :, :4])                # finished


def test_refusals_at_construction(models):
    """The three fixed sizes are refused by model.stream with the value named; a reverb that does not fit the ring keeps the
    packaged stream's text; slot mode stays with the packaged architecture."""
    half_hop = BANK_GIN + ("NeuralWaveshaping.control_hop = 64\nnoise_synth/FIRNoiseSynth.hop_length = 64\n"
                           "noise_synth/FIRNoiseSynth.ir_length = 128\nnoise_synth/TimeDistributedMLP.out_size = 65\n")
    m, _ = build_from_gin(half_hop)
    with pytest.raises(RuntimeError, match=r"control_hop = 64.*one-shot forward"):
        m.stream(1)
    y = m(torch.full((1, 1, 8), 200.0).cuda(), torch.randn(1, 2, 8).cuda())      # the one-shot forward serves it
    assert y.shape == (1, 512) and torch.isfinite(y).all()
    m, _ = build_from_gin(BANK_GIN + "noise_synth/FIRNoiseSynth.ir_length = 128\nnoise_synth/TimeDistributedMLP.out_size = 65\n")
    with pytest.raises(RuntimeError, match=r"ir_length = 128.*one-shot forward"):
        m.stream(1)
    m = copy.deepcopy(models("bank", False)[0])
    with torch.no_grad():
        m.noise_synth.window.copy_(torch.hamming_window(256))
    with pytest.raises(RuntimeError, match=r"window\[0\] = 0\.08.*one-shot forward"):
        m.stream(1)
    m, _ = build_from_gin(BANK_GIN + "NeuralWaveshaping.sample_rate = 22050\nHarmonicOscillator.sample_rate = 22050\nReverb.sr = 22050\n")
    assert m.reverb.ir.numel() == 44099 and not m._engine.specialised()
    with pytest.raises(RuntimeError, match="reverb history"):
        m.stream(1)
    with pytest.raises(RuntimeError, match="fused kernels"):
        models("bank", False)[0].stream(2, slots=True)


def test_refused_calls_touch_nothing(models):
    """Raw C ABI: a null state, f0 or out, K = 0, K > max_frames, `first` disagreeing with frames_seen and a state blob 4 bytes short
    return their codes before anything is launched - out still NaN, the state still its fill pattern - and a valid call right
    after gives the op's bits."""
    _lib = importlib.import_module(PKG + "._lib")
    engine = importlib.import_module(PKG + ".engine")
    binding, stream_ptr = engine.binding, engine.stream_ptr

    model, _ = models("bank", False)
    L = _lib.lib()
    r = model._engine.generic.model_desc()
    g, dev = r.struct, r.device
    B, K, maxf = 2, 2, 4
    nbytes = L.nws_g_stream_state_bytes(C.byref(g), B, maxf, g.ir_len, None)
    assert nbytes > 0
    f0, control, pu, nz = inputs("bank", B, K, 1)
    f0d, cd, pud, nzd = f0[:, 0].contiguous().cuda(), control.cuda(), pu.cuda(), torch.rand(128 * 8).cuda()
    M = L.nws_stream_out_samples(K, 1, 0)
    out = torch.full((B, M), float("nan"), device=dev)
    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    st = stream_ptr(dev)

    def call(state_ptr=None, nb=nbytes, f0p=None, outp=None, k=K, first=1, seen=0):
        return L.nws_g_stream_step(C.byref(g), None, None, None, state.data_ptr() if state_ptr is None else state_ptr, nb, B, maxf,
                                   f0d.data_ptr() if f0p is None else f0p, cd.data_ptr(), 2, k, first, 0, seen, 0,
                                   float(model.osc.sample_rate), pud.data_ptr(), r.rand_phase.data_ptr(), None, nzd.data_ptr(),
                                   nzd.numel(), out.data_ptr() if outp is None else outp, None, st)

    null = C.c_void_p(None)
    assert call(state_ptr=null) == BAD_ARG and call(f0p=null) == BAD_ARG and call(outp=null) == BAD_ARG
    assert call(k=0) == BAD_ARG and call(k=maxf + 1) == BAD_ARG
    assert call(first=1, seen=5) == BAD_ARG and call(first=0, seen=0) == BAD_ARG
    assert call(nb=nbytes - 4) == WORKSPACE
    assert L.nws_g_stream_state_bytes(C.byref(g), 0, maxf, g.ir_len, None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and bool((state == 0x5A).all())
    _lib.check(L.nws_stream_reset(state.data_ptr(), nbytes, st), "nws_stream_reset")
    assert call() == 0
    state2 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    out2 = torch.empty_like(out)
    binding().g_stream_step(r.gdesc, None, None, None, state2, maxf, f0d, cd, True, False, 0, 0, float(model.osc.sample_rate), pud,
                            r.rand_phase, None, nzd, out2, None)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, out2)
