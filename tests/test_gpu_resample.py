"""-m gpu: the resampler (csrc/resample.hip through both bindings) against the float64 restatement of the definition
(tests/resample_restatement.py).

Bound.  The GPU's max-abs error against the float64 restatement is at most 4x the max-abs error of the FLOAT32 restatement
on the same input (the same loop with fp64 weights and an fp32 running sum: resampy 0.2.2's arithmetic on float32 audio).
The kernel adds one rounding per term, the fp32 weight, of the size the running sum already makes (x sqrt 2); its order of
summation is free; the rest is the scatter of a maximum over a few thousand outputs.  The rule of the CMND test of
tests/test_gpu_pyin.py.  An all-zero row is exactly zero.

Shapes: the smallest at which each path of the kernel exists - see CASES."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import resample_restatement as rr
from conftest import ROOT
from gpu_util import record

pytestmark = pytest.mark.gpu

CASES = {
    "a_44100_16000": (44100, 16000, 6000),        # 13 periods of M = 441: both edges and an interior
    "b_48000_16000": (48000, 16000, 4001),        # L = 1, odd N
    "c_16000_48000": (16000, 48000, 1500),        # M = 1; 1500 periods: two tiles of 22 groups of 64
    "d_22050_16000": (22050, 16000, 3000),        # L = 320: three workgroups share a period tile
    "e_16000_44100": (16000, 44100, 1200),        # L = 441, even M = 160: the padded LDS rows, taps in two segments
    "f_8000_16000": (8000, 16000, 700),
    "g_44100_16000_short": (44100, 16000, 300),   # shorter than the taps: both wings clipped on every output
    "h_16000_16000": (16000, 16000, 1000),
    "i_44100_16000_two_tiles": (44100, 16000, 30000),   # 69 periods of M = 441: a second tile of 64 periods
    "j_192000_44100_direct": (192000, 44100, 3000),     # M = 640: 64 periods do not fit LDS, the one-thread-per-output kernel
    "k_16000_8000": (16000, 8000, 1001),                # M = 2: even and unpadded
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def _input(name):
    """(5, N) float32: tone + noise, zeros, unit impulses at 0, N - 1 and one interior sample"""
    sr_in, _, n = CASES[name]
    g = np.random.default_rng(7)
    x = np.zeros((5, n), dtype=np.float32)
    x[0] = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr_in) + 0.1 * g.standard_normal(n)
    x[2, 0] = x[3, n - 1] = x[4, (2 * n) // 3 + 1] = 1.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(name):
    sr_in, sr_out, _ = CASES[name]
    x = _input(name)
    return rr.resample(x, sr_in, sr_out), rr.resample(x, sr_in, sr_out, np.float32)


def _pre():
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import preprocess_audio as pre
    return pre


@functools.lru_cache(maxsize=None)
def _gpu(name):
    sr_in, sr_out, _ = CASES[name]
    y = _pre().resample_audio(torch.from_numpy(_input(name)).cuda(), sr_in, sr_out)
    torch.cuda.synchronize()
    return y.cpu().numpy()


ROWS = ("tone_noise", "zeros", "impulse_first", "impulse_last", "impulse_interior")


@pytest.mark.parametrize("name", NAMES)
def test_within_four_times_the_float32_restatement(name):
    sr_in, sr_out, n = CASES[name]
    y, (y64, y32) = _gpu(name), _ref(name)
    assert y.dtype == np.float32 and y.shape == y64.shape == (5, (n * rr.config(sr_in, sr_out).L) // rr.config(sr_in, sr_out).M)
    assert np.isfinite(y).all()
    errs = {}
    for i, row in enumerate(ROWS):
        err = float(np.abs(y[i].astype(np.float64) - y64[i]).max())
        err32 = float(np.abs(y32[i].astype(np.float64) - y64[i]).max())
        errs[row] = (err, err32)
        print(name, row, "max abs err: gpu", err, "float32 restatement", err32)
    record("resample_" + name, outputs=int(y.shape[1]), max_abs_err_gpu=errs["tone_noise"][0],
           max_abs_err_float32_restatement=errs["tone_noise"][1],
           **{"gpu_over_float32_" + row: (e / e32 if e32 else 0.0) for row, (e, e32) in errs.items()})
    assert np.all(y[1] == 0)
    assert np.abs(y64[0]).max() > 0.3 and all(np.abs(y64[i]).max() > 1e-3 for i in (2, 3, 4))      # not vacuous
    for row, (err, err32) in errs.items():
        assert err <= 4 * err32, (name, row, err, err32)


def test_batch_rows_equal_their_single_row_results_bit_for_bit():
    pre = _pre()
    g = np.random.default_rng(3)
    n = CASES["a_44100_16000"][2]
    x = np.stack([_input("a_44100_16000")[0], *(0.2 * g.standard_normal((3, n))).astype(np.float32), _input("a_44100_16000")[4]])
    a = torch.from_numpy(x).cuda()
    whole = pre.resample_audio(a, 44100, 16000)
    assert whole.shape == (5, (n * 160) // 441)
    for i in range(5):
        assert torch.equal(whole[i:i + 1], pre.resample_audio(a[i:i + 1].clone(), 44100, 16000)), i
        assert torch.equal(whole[i], pre.resample_audio(a[i].clone(), 44100, 16000)), i
    # a longer batch of the same rows: tiles of other rows around them change nothing
    again = pre.resample_audio(torch.cat([a, a, a[:3]]), 44100, 16000)
    assert torch.equal(again[:5], whole) and torch.equal(again[5:10], whole) and torch.equal(again[10:], whole[:3])


def test_both_bindings_and_the_front_end_agree_bit_for_bit():
    pre = _pre()
    from nws_amd import _cops, build
    torch.ops.load_library(build.OPS_LIB)              # the op library, whichever binding the package itself uses
    sr_in, sr_out, _ = CASES["a_44100_16000"]
    x = _input("a_44100_16000")
    a = torch.from_numpy(x).cuda()
    bank_ops, bank_c = torch.ops.newt_hip.resample_bank(sr_in, sr_out), _cops.CtypesOps().resample_bank(sr_in, sr_out)
    assert bank_ops.device.type == "cpu" and bank_ops.dtype == torch.float32 and bank_ops.shape == rr.dims(sr_in, sr_out)[0:3:2]
    assert torch.equal(bank_ops, bank_c)
    bank = bank_ops.cuda()
    y_ops = torch.ops.newt_hip.resample(a, bank, sr_in, sr_out)
    y_c = _cops.CtypesOps().resample(a, bank, sr_in, sr_out)
    assert torch.equal(y_ops, y_c) and np.array_equal(y_ops.cpu().numpy(), _gpu("a_44100_16000"))
    y_np = pre.resample_audio(x[0], sr_in, sr_out)                     # numpy in, numpy float32 out, as the reference
    assert isinstance(y_np, np.ndarray) and y_np.dtype == np.float32 and np.array_equal(y_np, y_ops[0].cpu().numpy())
    y_np = pre.resample_audio(x[0].astype(np.float64), float(sr_in), float(sr_out))
    assert y_np.dtype == np.float32 and np.array_equal(y_np, y_ops[0].cpu().numpy())
    y_t = pre.resample_audio(a[0], sr_in, sr_out)
    assert y_t.is_cuda and y_t.shape == y_ops.shape[1:] and torch.equal(y_t, y_ops[0])
    # a bank of other rates, a CPU bank and an empty result are refused by both bindings
    other = torch.ops.newt_hip.resample_bank(48000, 16000).cuda()
    for b in (torch.ops.newt_hip, _cops.CtypesOps()):
        with pytest.raises(RuntimeError, match="bank"):
            b.resample(a, other, sr_in, sr_out)
        with pytest.raises(RuntimeError):
            b.resample(a, bank_ops, sr_in, sr_out)
        with pytest.raises(RuntimeError, match="give no sample"):
            b.resample(a[:, :2].contiguous(), bank, sr_in, sr_out)
        with pytest.raises(RuntimeError, match="unsupported rates"):
            b.resample_bank(191999, 8000)


def test_c_abi_codes_and_a_valid_call():
    _pre()
    from nws_amd import _lib
    L = _lib.lib()
    sr_in, sr_out, n = CASES["a_44100_16000"]
    a = torch.from_numpy(_input("a_44100_16000")).cuda()
    bank = torch.empty(rr.dims(sr_in, sr_out)[0], rr.dims(sr_in, sr_out)[2], dtype=torch.float32)
    assert L.nws_resample_bank(sr_in, sr_out, bank.data_ptr()) == 0
    bank = bank.cuda()
    n_out = L.nws_resample_length(n, sr_in, sr_out)
    y = torch.full((5, n_out), 7.0, device="cuda")
    args = (a.data_ptr(), 5, n, sr_in, sr_out, bank.data_ptr(), y.data_ptr(), None)
    assert L.nws_resample(None, *args[1:]) == -2 and L.nws_resample(*args[:5], None, *args[6:]) == -2
    assert L.nws_resample(*args[:6], None, None) == -2
    assert L.nws_resample(args[0], 0, *args[2:]) == -2
    assert L.nws_resample(*args[:3], 191999, 8000, *args[5:]) == -1
    assert L.nws_resample(*args[:3], 0, 16000, *args[5:]) == -1
    torch.cuda.synchronize()
    assert torch.all(y == 7.0)                                          # nothing was launched
    assert L.nws_resample(*args) == 0
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), _gpu("a_44100_16000"))


def test_timbre_transfer_script_resamples_a_stereo_file(tmp_path):
    n = 22050
    t = np.arange(n) / 22050.0
    tone = 0.3 * np.sin(2 * np.pi * 220.0 * t) * np.minimum(1.0, 10 * t)
    stereo = np.stack([tone, 0.5 * tone[::-1]], axis=1)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    wavfile.write(src, 22050, np.round(stereo * 32767.0).astype(np.int16))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "timbre_transfer.py"), src, dst, "--resample", "--use-fastnewt"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    n16 = (n * 320) // 441
    sr, y = wavfile.read(dst)
    assert sr == 16000 and y.shape == (n16,) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() > 1e-4
    assert "median F0 2" in r.stdout, r.stdout                  # 220 Hz within a bin or two
    r = subprocess.run(cmd + ["--output-rate", "22050"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    sr, y = wavfile.read(dst)
    assert sr == 22050 and y.shape == ((n16 * 441) // 320,) and y.dtype == np.float32 and np.isfinite(y).all()
    assert np.abs(y).max() > 1e-4


def test_times_on_the_bench_clips_one_minute_and_an_upsampling():
    """no bar: there is no earlier implementation to compare with.  hipEvents on the launch stream, mean of 3, recorded for
    DESIGN.md 3.10"""
    pre = _pre()
    g = torch.Generator(device="cuda").manual_seed(3)
    for tag, shape, sr_in, sr_out in (("64x4s_44100_16000", (64, 176400), 44100, 16000), ("1x60s_48000_16000", (1, 60 * 48000), 48000, 16000),
                                      ("64x4s_16000_48000", (64, 64000), 16000, 48000)):
        a = 0.3 * torch.randn(shape, device="cuda", generator=g)
        y = pre.resample_audio(a, sr_in, sr_out)                       # the bank's upload is not part of the time
        assert y.shape == (shape[0], rr.length(shape[1], sr_in, sr_out))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            pre.resample_audio(a, sr_in, sr_out)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / 3
        taps = rr.dims(sr_in, sr_out)[2]
        record("resample_time_" + tag, ms=ms, outputs=int(y.numel()), taps=taps, gfma_per_s=y.numel() * taps / (ms * 1e-3) / 1e9,
               x_realtime=a.numel() / sr_in / (ms * 1e-3))
        print(tag, ms, "ms")
        assert np.isfinite(ms) and ms > 0
