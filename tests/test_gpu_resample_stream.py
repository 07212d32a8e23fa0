"""-m gpu: the streaming resampler (csrc/resample_stream.hip through both bindings and streaming.StreamResampler) against the
float64 restatements (tests/resample_restatement.py, tests/resample_stream_restatement.py).

Bound: the offline test's (tests/test_gpu_resample.py) - per row, the max-abs error against the float64 restatement of the
WHOLE signal is at most 4x that of the float32 restatement on the same row; an all-zero row is exactly zero.
Exact: any chunking of the same input gives the same bits; a row's bits do not depend on the other rows; both bindings and the
captured hop give the same bits as eager pushes.

Shapes: the smallest at which each path exists - see CASES."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_restatement as rr
import resample_stream_restatement as rs
from conftest import ROOT
from gpu_util import build_model, record

pytestmark = pytest.mark.gpu

ROWS = ("tone_noise", "zeros", "impulse_first", "impulse_last", "impulse_interior")


def _hops(n, hop):
    return [hop] * (n // hop) + ([n % hop] if n % hop else [])


def _ragged(n, taps):
    """a fixed list with 1, a prime below 64, 256 and one value above `taps` in front, the same sizes in turn up to n"""
    out = [1, 37, 256, taps + 9]
    assert sum(out) < n
    for size in (37, 1, 256) * n:
        if sum(out) == n:
            break
        out.append(min(size, n - sum(out)))
    return out


def _case(sr_in, sr_out, n, *chunkings):
    taps = rr.config(sr_in, sr_out).taps
    return sr_in, sr_out, n, {tag: (_ragged(n, taps) if c == "ragged" else [n] if c == "whole" else c) for tag, c in chunkings}


CASES = {
    # L = 3, M = 1; chunks longer than the history of 126 samples
    "a_16000_48000": _case(16000, 48000, 1024, ("whole", "whole"), ("hops", _hops(1024, 256)), ("ragged", "ragged")),
    # 441 weight rows; 705 / 706 outputs per hop over one full cycle of 5 hops
    "b_16000_44100": _case(16000, 44100, 1280, ("whole", "whole"), ("hops", _hops(1280, 256)), ("ragged", "ragged")),
    # L = 1, 383 taps
    "c_48000_16000": _case(48000, 16000, 2304, ("whole", "whole"), ("hops", _hops(2304, 768)), ("ragged", "ragged")),
    # pushes that emit nothing; a history longer than the chunk
    "d_44100_16000": _case(44100, 16000, 2000, ("whole", "whole"), ("hops", _hops(2000, 441)), ("ones", [1] * 600 + [1400])),
    # L = M = 1
    "e_16000_16000": _case(16000, 16000, 500, ("whole", "whole"), ("hops", _hops(500, 7))),
    # N < right: every output comes from the final push
    "f_44100_16000_short": _case(44100, 16000, 100, ("whole", "whole"), ("hops", _hops(100, 33))),
    # one push above max_chunk, split inside push
    "g_48000_16000_long": _case(48000, 16000, 10000, ("whole", "whole"), ("hops", _hops(10000, 768))),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def _input(name):
    """(5, N) float32: tone + noise, zeros, unit impulses at 0, N - 1 and one interior sample (the offline test's rows)"""
    sr_in, _, n, _ = CASES[name]
    g = np.random.default_rng(7)
    x = np.zeros((5, n), dtype=np.float32)
    x[0] = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr_in) + 0.1 * g.standard_normal(n)
    x[2, 0] = x[3, n - 1] = x[4, (2 * n) // 3 + 1] = 1.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(name):
    sr_in, sr_out, _, _ = CASES[name]
    x = _input(name)
    return rr.resample(x, sr_in, sr_out), rr.resample(x, sr_in, sr_out, np.float32)


def _streaming():
    import nws_amd  # noqa: F401
    from nws_amd import streaming
    return streaming


def _push_all(s, x, chunks):
    """x (B, N) on the device through stream `s` in `chunks`, then flush(): (columns per push, the flush's included; the
    concatenation, copied out push by push)"""
    counts, outs, at = [], [], 0
    for n in chunks:
        o = s.push(x[:, at:at + n])
        at += n
        counts.append(int(o.shape[1]))
        outs.append(o.clone())
    o = s.flush()
    counts.append(int(o.shape[1]))
    outs.append(o.clone())
    assert at == x.shape[1] and s.samples_in == at and s.samples_out == sum(counts) and s.finished
    return counts, torch.cat(outs, dim=1)


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """{chunking: (columns per push, (5, n_out) numpy)} of a case, every chunking through a stream of its own; check() after each"""
    sr_in, sr_out, _, chunkings = CASES[name]
    x = torch.from_numpy(_input(name)).cuda()
    res = {}
    for tag, chunks in chunkings.items():
        s = _streaming().StreamResampler(sr_in, sr_out, 5)
        counts, y = _push_all(s, x, chunks)
        s.check()
        res[tag] = (counts, y.cpu().numpy())
    return res


@pytest.mark.parametrize("name", NAMES)
def test_within_four_times_the_float32_restatement(name):
    sr_in, sr_out, n, chunkings = CASES[name]
    c = rr.config(sr_in, sr_out)
    y, (y64, y32) = _gpu(name)[list(chunkings)[-1]][1], _ref(name)
    assert y.dtype == np.float32 and y.shape == y64.shape == (5, (n * c.L) // c.M)
    assert np.isfinite(y).all()
    errs = {}
    for i, row in enumerate(ROWS):
        err = float(np.abs(y[i].astype(np.float64) - y64[i]).max())
        err32 = float(np.abs(y32[i].astype(np.float64) - y64[i]).max())
        errs[row] = (err, err32)
        print(name, row, "max abs err: gpu", err, "float32 restatement", err32)
    record("resample_stream_" + name, outputs=int(y.shape[1]), max_abs_err_gpu=errs["tone_noise"][0],
           max_abs_err_float32_restatement=errs["tone_noise"][1],
           **{"gpu_over_float32_" + row: (e / e32 if e32 else 0.0) for row, (e, e32) in errs.items()})
    assert np.all(y[1] == 0)
    assert np.abs(y64[0]).max() > 0.3 and all(np.abs(y64[i]).max() > 1e-3 for i in (2, 3, 4))      # not vacuous
    for row, (err, err32) in errs.items():
        assert err <= 4 * err32, (name, row, err, err32)


@pytest.mark.parametrize("name", NAMES)
def test_every_chunking_gives_the_same_bits_and_the_counts_of_the_definition(name):
    sr_in, sr_out, n, chunkings = CASES[name]
    c = rr.config(sr_in, sr_out)
    res = _gpu(name)
    first = res[list(chunkings)[0]][1]
    for tag, chunks in chunkings.items():
        counts, y = res[tag]
        assert np.array_equal(y.view(np.int32), first.view(np.int32)), (name, tag)
        seen, want = 0, []
        for k in chunks:                 # a push above max_chunk is one push to the caller
            want.append(rs.emitted(seen + k, sr_in, sr_out) - rs.emitted(seen, sr_in, sr_out))
            seen += k
        want.append(rr.length(n, sr_in, sr_out) - rs.emitted(n, sr_in, sr_out))
        assert counts == want, (name, tag)
    # the lists reach what they are for
    if "ragged" in chunkings:
        assert min(chunkings["ragged"]) < c.taps - 1 < max(chunkings["ragged"]) and {1, 37, 256} <= set(chunkings["ragged"])
    if name == "b_16000_44100":
        assert res["hops"][0][0] == 530 and set(res["hops"][0][1:5]) == {705, 706} and len(res["hops"][0]) == 6
    if name == "d_44100_16000":
        assert res["ones"][0][:c.right] == [0] * c.right and set(res["ones"][0][:600]) == {0, 1} and 441 > c.taps - 1 > 1
    if name == "f_44100_16000_short":
        assert n < c.right and all(r[0][:-1] == [0] * (len(r[0]) - 1) and r[0][-1] == 36 for r in res.values())
    if name == "g_48000_16000_long":
        assert n > _streaming().StreamResampler(sr_in, sr_out, 1).max_chunk == 4096


@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_their_single_row_streams_bit_for_bit(name):
    sr_in, sr_out, _, chunkings = CASES[name]
    tag = list(chunkings)[1]
    whole = _gpu(name)[tag][1]
    x = torch.from_numpy(_input(name)).cuda()
    for i in range(5):
        s = _streaming().StreamResampler(sr_in, sr_out, 1)
        _, y = _push_all(s, x[i:i + 1].clone(), chunkings[tag])
        s.check()
        assert np.array_equal(y.cpu().numpy().view(np.int32), whole[i:i + 1].view(np.int32)), (name, i)


@pytest.mark.parametrize("name", ["a_16000_48000", "d_44100_16000"])
def test_both_bindings_give_the_same_bits(name):
    _streaming()
    from nws_amd import _cops, _lib, build
    from nws_amd.data.utils import preprocess_audio as pre
    torch.ops.load_library(build.OPS_LIB)              # the op library, whichever binding the package itself uses
    sr_in, sr_out, n, chunkings = CASES[name]
    tag = list(chunkings)[-1]
    x = torch.from_numpy(_input(name)).cuda()
    bank = pre._bank(sr_in, sr_out, x.device)
    L = _lib.lib()
    got = []
    for b in (torch.ops.newt_hip, _cops.CtypesOps()):
        state = torch.empty(L.nws_resample_stream_state_bytes(5, sr_in, sr_out), dtype=torch.uint8, device="cuda")
        b.resample_stream_reset(state, 5, sr_in, sr_out)
        outs, seen, at = [], 0, 0
        for k, final in [(k, False) for k in chunkings[tag]] + [(0, True)]:
            out = torch.full((5, L.nws_resample_stream_max_out(k, sr_in, sr_out, int(final)) + 3), 7.0, device="cuda")
            b.resample_stream_step(state, bank, sr_in, sr_out, x[:, at:at + k].contiguous(), final, out)
            m = rs.emitted(seen + k, sr_in, sr_out, final) - rs.emitted(seen, sr_in, sr_out)
            assert torch.all(out[:, m:] == 7.0)                       # the rest of the row is left untouched
            outs.append(out[:, :m])
            seen, at = seen + k, at + k
        got.append(torch.cat(outs, dim=1))
    assert torch.equal(got[0], got[1])
    assert np.array_equal(got[0].cpu().numpy().view(np.int32), _gpu(name)[tag][1].view(np.int32))


def test_captured_hop_equals_eager_pushes():
    sr_in, sr_out = 16000, 44100
    g = torch.Generator(device="cuda").manual_seed(5)
    x = 0.3 * torch.randn((2, 10 * 256), device="cuda", generator=g)
    eager = _streaming().StreamResampler(sr_in, sr_out, 2, graph=False)
    want = [eager.push(x[:, i * 256:(i + 1) * 256]).clone() for i in range(10)]
    s = _streaming().StreamResampler(sr_in, sr_out, 2)
    for i in range(2):                                                   # warm-up pushes
        assert torch.equal(s.push(x[:, i * 256:(i + 1) * 256]), want[i])
    x_in, out = s.static_io(256)
    assert x_in.shape == (2, 256) and out.shape == (2, 706)
    counts = []
    for i in range(2, 10):
        x_in.copy_(x[:, i * 256:(i + 1) * 256])
        y = s.hop()
        counts.append(int(y.shape[1]))
        assert y.data_ptr() == out.data_ptr() and torch.equal(y, want[i]), i
    assert counts == [rs.emitted(256 * (i + 1), sr_in, sr_out) - rs.emitted(256 * i, sr_in, sr_out) for i in range(2, 10)]
    assert set(counts) == {705, 706} and counts[:3] == counts[5:8]     # the pattern repeats every 5 hops
    assert s._graphs[256][0] is not None and eager._graphs == {}
    s.check()
    eager.check()
    assert torch.equal(s.flush(), eager.flush())


def test_reset_and_refusals_leave_the_state_alone():
    streaming = _streaming()
    from nws_amd import _cops
    from nws_amd.data.utils import preprocess_audio as pre
    from nws_amd.engine import binding
    sr_in, sr_out = 16000, 48000
    g = torch.Generator(device="cuda").manual_seed(9)
    x = 0.3 * torch.randn((3, 700), device="cuda", generator=g)
    s = streaming.StreamResampler(sr_in, sr_out, 3)
    assert s.latency_samples == 63 and s.samples_in == s.samples_out == 0
    _, first = _push_all(s, x, [300, 400])
    with pytest.raises(RuntimeError, match="stream already finished"):
        s.push(x[:, :10])
    with pytest.raises(RuntimeError, match="stream already finished"):
        s.flush()
    s.reset()
    assert s.samples_in == s.samples_out == 0 and not s.finished
    s.check()
    _, again = _push_all(s, x, [300, 400])
    assert torch.equal(first, again)
    # refusals in the middle of a stream: the next valid push equals the undisturbed stream's
    s.reset()
    a = s.push(x[:, :300]).clone()
    other = pre._bank(48000, 16000, x.device)
    for b in (binding(), _cops.CtypesOps()):
        with pytest.raises(RuntimeError, match="bank does not belong to these rates"):
            b.resample_stream_step(s._state, other, sr_in, sr_out, x[:, 300:].contiguous(), False, torch.empty((3, 1200), device="cuda"))
        with pytest.raises(RuntimeError, match=r"out: expected \(3, >= 1200\)"):
            b.resample_stream_step(s._state, s._bank, sr_in, sr_out, x[:, 300:].contiguous(), False, torch.empty((3, 1199), device="cuda"))
        with pytest.raises(RuntimeError, match="state does not belong to a stream of B = 2"):
            b.resample_stream_step(s._state, s._bank, sr_in, sr_out, x[:2, 300:].contiguous(), False, torch.empty((2, 1200), device="cuda"))
        with pytest.raises(RuntimeError, match="empty chunk"):
            b.resample_stream_step(s._state, s._bank, sr_in, sr_out, x[:, :0].contiguous(), False, torch.empty((3, 1200), device="cuda"))
    with pytest.raises(RuntimeError, match="empty chunk"):
        s.push(x[:, :0])
    with pytest.raises(RuntimeError, match="chunk lives on cpu"):
        s.push(x[:, 300:].cpu())
    with pytest.raises(RuntimeError, match="chunk: expected"):
        s.push(x[:, 300:].double())
    with pytest.raises(RuntimeError, match="state does not belong to a stream of B = 4"):
        s.push(torch.zeros((4, 400), device="cuda"))
    assert s.samples_in == 300 and not s.finished
    s.check()
    b_ = torch.cat([a, s.push(x[:, 300:]), s.flush()], dim=1)
    assert torch.equal(b_, first)
    with pytest.raises(RuntimeError, match="unsupported stream"):
        streaming.StreamResampler(1000000, 2500, 1)


def test_model_stream_into_the_converter():
    model = build_model(fast=True)
    g = torch.Generator().manual_seed(4)
    f0 = (220 + 20 * torch.rand((1, 1, 12), generator=g)).cuda()
    control = torch.randn((1, 2, 12), generator=g).cuda()
    with torch.no_grad():
        ms = model.stream(1)
        rs48 = _streaming().StreamResampler(16000, 48000, 1)
        audio, out = [], []
        for i in range(6):
            a = ms.push(f0[:, :, 2 * i:2 * i + 2], control[:, :, 2 * i:2 * i + 2], final=i == 5).clone()
            audio.append(a)
            out.append(rs48.push(a, final=i == 5).clone())
    audio, out = torch.cat(audio, dim=1), torch.cat(out, dim=1)
    assert audio.shape == (1, 12 * 128) and out.shape == (1, 3 * 12 * 128) and float(audio.abs().max()) > 1e-4
    rs48.check()
    one = _streaming().StreamResampler(16000, 48000, 1)
    assert torch.equal(out, torch.cat([one.push(audio), one.flush()], dim=1))


def test_time_streaming_script_with_and_without_an_output_rate(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "time_streaming.py"), "--num-hops", "20"]
    old = {"stream", "batch", "hop_samples", "graph", "static_io", "hops", "python_gc", "slots", "events", "p50_us", "p99_us", "max_us",
           "wall_p50_us", "wall_p99_us", "x_realtime_p50"}
    new = {"output_rate", "output_samples", "converter_p50_us", "converter_p99_us", "p50_with_converter_us", "p99_with_converter_us"}
    for extra, want in ((["--output-rate", "48000"], old | new), ([], old)):
        path = str(tmp_path / ("with.json" if extra else "without.json"))
        r = subprocess.run(cmd + extra + ["--json-out", path], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res = json.loads(open(path).read().strip())
        assert set(res) == want, set(res) ^ want
        assert res["hops"] == 20 and res["p50_us"] > 0
        if extra:
            assert res["output_rate"] == 48000 and res["output_samples"] == 20 * 768
            assert res["converter_p50_us"] > 0 and res["p50_with_converter_us"] >= res["p50_us"]
