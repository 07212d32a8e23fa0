"""-m gpu: the MFCC feature (csrc/mfcc.hip through both bindings) against the float64 restatement of the definition
(tests/mfcc_restatement.py).

Bound.  The rule of tests/test_gpu_resample.py with the output's own rounding added:
    max|gpu - f64| <= 4 max|float32 restatement - f64| + ulp32(max|f64|).
The float32 restatement is the same chain in float32 with the windowed DFT as a float32 matrix product - sums of n_fft
fp32 terms, the kernel's kind of transform; the kernel's order of summation is free (a 512-step chain of two products per
step), which on a maximum over a few thousand outputs is worth a small factor.  The second term is the float32 rounding of
the result itself, the whole error where c[0] sits near -1131 (an all-zero utterance).

Measured on the MI355X (gpu | float32 restatement, max abs error against float64): 1.0e-5 | 1.3e-5 (noise) ... 1.29e-3 | 6.6e-4 (vibrato tone, the
largest: 1.95 x); every pair is in DESIGN.md 3.11.

Shapes: the smallest at which each path of the kernels exists - see CASES."""
import functools

import numpy as np
import pytest
import torch

import mfcc_restatement as mr
from gpu_util import record

pytestmark = pytest.mark.gpu

SHIPPED = (16000, 1024, 128, 16, 128)          # sample_rate, n_fft, hop_length, n_mfcc, n_mels


def _vibrato(n, sr=16000, f0=220.0):
    t = np.arange(n) / sr
    phase = 2 * np.pi * f0 * (t - 0.01 * np.cos(2 * np.pi * 5.0 * t) / (2 * np.pi * 5.0))
    return sum(a * np.sin(h * phase) for h, a in ((1, 0.4), (2, 0.2), (3, 0.1)))


def _make(name):
    g = np.random.default_rng(11)
    if name == "vibrato_tone":
        return _vibrato(6000) + 1e-3 * g.standard_normal(6000)
    if name == "pure_tone":
        return 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(5000) / 16000.0)
    if name == "noise_odd":
        return 0.3 * g.standard_normal(4099)
    if name == "click":
        x = np.zeros(6001)
        x[3000] = 1.0
        return x
    if name == "zeros":
        return np.zeros(5000)
    if name == "noise_22050_40":
        return 0.3 * g.standard_normal(3001)
    if name == "noise_2048_20":
        return 0.3 * g.standard_normal(9000)
    if name == "quiet_then_loud":
        return np.concatenate([1e-3 * g.standard_normal(3000), 0.5 * g.standard_normal(3000)])
    if name == "silent_then_loud":
        return np.concatenate([1e-6 * g.standard_normal(3000), 0.5 * g.standard_normal(3000)])
    raise KeyError(name)


CASES = {
    "vibrato_tone": SHIPPED,                   # 47 frames: crosses the 32-frame tile of the power pass
    "pure_tone": SHIPPED,                      # most dB entries on the clip
    "noise_odd": SHIPPED,                      # odd length, 33 frames: one frame in a second tile
    "click": SHIPPED,
    "zeros": SHIPPED,
    "noise_22050_40": (22050, 256, 100, 13, 40),
    "noise_2048_20": (16000, 2048, 512, 20, 128),        # two groups of sixteen DCT coefficients
    "quiet_then_loud": SHIPPED,                # the loud half sets the clip level for the quiet half (54 dB below: not reached)
    "silent_then_loud": SHIPPED,               # 114 dB below: the quiet half sits on the clip the loud half sets
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def _input(name):
    x = np.ascontiguousarray(_make(name), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(name):
    sr, n_fft, hop, n_mfcc, n_mels = CASES[name]
    x = _input(name)
    return mr.mfcc(x, sr, n_fft, hop, n_mfcc, n_mels), mr.mfcc_float32(x, sr, n_fft, hop, n_mfcc, n_mels)


def _me():
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import mfcc_extraction as me
    return me


@functools.lru_cache(maxsize=None)
def _gpu(name):
    sr, n_fft, hop, n_mfcc, n_mels = CASES[name]
    y = _me().mfcc_frames(torch.from_numpy(_input(name)).cuda()[None], sr, n_fft, hop, n_mfcc, n_mels)
    torch.cuda.synchronize()
    return y.cpu().numpy()[0]


def _operands(name):
    from nws_amd.data.utils.loudness_extraction import _dft_operand
    sr, n_fft, hop, n_mfcc, n_mels = CASES[name]
    me = _me()
    dev = torch.device("cuda", torch.cuda.current_device())
    return _dft_operand(n_fft, dev), me._table((float(sr), n_fft, n_mfcc, n_mels), dev)


def test_restatement_cases_are_not_vacuous():
    c64, _ = _ref("vibrato_tone")
    assert np.abs(c64).max() > 100
    assert mr.clipped_share(_input("pure_tone"), 16000, 1024, 128) > 0.5
    for name in ("noise_odd", "noise_22050_40", "noise_2048_20"):
        sr, n_fft, hop, _, n_mels = CASES[name]
        assert mr.clipped_share(_input(name), sr, n_fft, hop, n_mels) == 0.0, name
    assert mr.clipped_share(_input("quiet_then_loud"), 16000, 1024, 128) == 0.0
    assert 0.2 < mr.clipped_share(_input("silent_then_loud"), 16000, 1024, 128) < 0.8
    assert [1 + _input(n).size // CASES[n][2] for n in ("vibrato_tone", "noise_odd")] == [47, 33]


@pytest.mark.parametrize("name", NAMES)
def test_within_four_times_the_float32_restatement(name):
    from nws_amd import _cops, build
    torch.ops.load_library(build.OPS_LIB)              # the op library, whichever binding the package itself uses
    sr, n_fft, hop, n_mfcc, n_mels = CASES[name]
    x = _input(name)
    y, (c64, c32) = _gpu(name), _ref(name)
    assert y.dtype == np.float32 and y.shape == c64.shape == (n_mfcc, 1 + x.size // hop)
    assert np.isfinite(y).all()
    err = float(np.abs(y.astype(np.float64) - c64).max())
    err32 = float(np.abs(c32.astype(np.float64) - c64).max())
    ulp = float(np.spacing(np.float32(np.abs(c64).max())))
    print(name, "max abs err: gpu", err, "float32 restatement", err32, "ulp32 of the largest value", ulp)
    record("mfcc_" + name, frames=int(y.shape[1]), max_abs_err_gpu=err, max_abs_err_float32_restatement=err32,
           ulp32_of_largest=ulp, largest=float(np.abs(c64).max()))
    # both bindings give the front end's bits
    a = torch.from_numpy(x).cuda()[None]
    dft, table = _operands(name)
    for b in (torch.ops.newt_hip, _cops.CtypesOps()):
        assert np.array_equal(b.mfcc(a, dft, table, float(sr), n_fft, hop, n_mfcc, n_mels)[0].cpu().numpy(), y), name
    assert err <= 4 * err32 + ulp, (name, err, err32, ulp)


def test_zero_row_is_exact():
    y = _gpu("zeros")
    assert (y[0] == np.float32(-100.0 * np.sqrt(128.0))).all()
    assert (y[1:] == 0).all()


def test_batch_rows_equal_their_single_row_results_bit_for_bit():
    me = _me()
    g = np.random.default_rng(5)
    x = np.stack([_input("vibrato_tone"), (0.2 * g.standard_normal(6000)).astype(np.float32),
                  np.float32(1e-3) * _input("vibrato_tone")]).astype(np.float32)
    a = torch.from_numpy(x).cuda()
    whole = me.mfcc_frames(a, *SHIPPED)
    assert whole.shape == (3, 16, 47)
    for i in range(3):
        assert torch.equal(whole[i:i + 1], me.mfcc_frames(a[i:i + 1].clone(), *SHIPPED)), i
    assert np.array_equal(whole[0].cpu().numpy(), _gpu("vibrato_tone"))
    # the scaled row has a maximum of its own (60 dB lower): it is held to the restatement of the scaled input by the same rule
    c64, c32 = (f(x[2], *SHIPPED) for f in (mr.mfcc, mr.mfcc_float32))
    err, err32 = np.abs(whole[2].cpu().numpy() - c64).max(), np.abs(c32 - c64).max()
    print("scaled row: gpu", err, "float32 restatement", err32)
    assert np.abs(c64[0] - _ref("vibrato_tone")[0][0]).min() > 500      # 60 dB sqrt(128) = 679, less what the amin floor takes
    assert err <= 4 * err32 + float(np.spacing(np.float32(np.abs(c64).max())))
    again = me.mfcc_frames(torch.cat([a, a[:2]]), *SHIPPED)
    assert torch.equal(again[:3], whole) and torch.equal(again[3:], whole[:2])


def test_both_bindings_and_the_front_end_agree_bit_for_bit():
    me = _me()
    from nws_amd import _cops, build
    torch.ops.load_library(build.OPS_LIB)
    sr, n_fft, hop, n_mfcc, n_mels = SHIPPED
    cfg = (float(sr), n_fft, n_mfcc, n_mels)
    t_ops, t_c = torch.ops.newt_hip.mfcc_table(*cfg), _cops.CtypesOps().mfcc_table(*cfg)
    assert t_ops.device.type == "cpu" and t_ops.dtype == torch.float32 and t_ops.dim() == 1 and torch.equal(t_ops.view(torch.int32), t_c.view(torch.int32))
    x = _input("vibrato_tone")
    a = torch.from_numpy(x).cuda()
    dft, _ = _operands("vibrato_tone")
    table = t_ops.cuda()
    y_ops = torch.ops.newt_hip.mfcc(a[None], dft, table, *cfg[:2], hop, n_mfcc, n_mels)
    y_c = _cops.CtypesOps().mfcc(a[None], dft, table, *cfg[:2], hop, n_mfcc, n_mels)
    assert torch.equal(y_ops, y_c) and np.array_equal(y_ops[0].cpu().numpy(), _gpu("vibrato_tone"))
    y_np = me.extract_mfcc(x, sr, n_fft, hop, n_mfcc)                  # numpy in, numpy (n_mfcc, T) float32 out, as the reference
    assert isinstance(y_np, np.ndarray) and y_np.dtype == np.float32 and np.array_equal(y_np, y_ops[0].cpu().numpy())
    y_np = me.extract_mfcc(x.astype(np.float64), float(sr), n_fft, hop, n_mfcc)
    assert y_np.dtype == np.float32 and np.array_equal(y_np, y_ops[0].cpu().numpy())
    y_t = me.extract_mfcc(a, sr, n_fft, hop, n_mfcc)
    assert y_t.is_cuda and y_t.shape == (n_mfcc, 47) and torch.equal(y_t, y_ops[0])
    y_b = me.extract_mfcc(torch.stack([a, a]), sr, n_fft, hop, n_mfcc)
    assert y_b.shape == (2, n_mfcc, 47) and torch.equal(y_b[0], y_ops[0]) and torch.equal(y_b[1], y_ops[0])
    # a table of another configuration, a CPU table, a short row and an unsupported configuration are refused by both bindings
    other = torch.ops.newt_hip.mfcc_table(float(sr), n_fft, 20, n_mels).cuda()
    for b in (torch.ops.newt_hip, _cops.CtypesOps()):
        with pytest.raises(RuntimeError, match="table"):
            b.mfcc(a[None], dft, other, *cfg[:2], hop, n_mfcc, n_mels)
        with pytest.raises(RuntimeError):
            b.mfcc(a[None], dft, t_ops, *cfg[:2], hop, n_mfcc, n_mels)
        with pytest.raises(RuntimeError, match="unsupported size"):
            b.mfcc(a[None, :512].contiguous(), dft, table, *cfg[:2], hop, n_mfcc, n_mels)
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            b.mfcc_table(float(sr), n_fft, 129, n_mels)
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            b.mfcc_table(0.0, n_fft, n_mfcc, n_mels)


def test_c_abi_refusals_launch_nothing_and_a_valid_call():
    _me()
    from nws_amd import _lib
    L = _lib.lib()
    sr, n_fft, hop, n_mfcc, n_mels = SHIPPED
    a = torch.from_numpy(_input("vibrato_tone")).cuda()[None]
    dft, table = _operands("vibrato_tone")
    nbytes = L.nws_mfcc_workspace_bytes(1, 6000, n_fft, hop, n_mels)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    y = torch.full((1, n_mfcc, 47), 7.0, device="cuda")
    args = [a.data_ptr(), 1, 6000, float(sr), n_fft, hop, n_mfcc, n_mels, dft.data_ptr(), table.data_ptr(), y.data_ptr(), ws.data_ptr(),
            nbytes, None]
    torch.cuda.synchronize()
    for i in (0, 8, 9, 10, 11):
        bad = list(args)
        bad[i] = None
        assert L.nws_mfcc(*bad) == -2, i
    assert L.nws_mfcc(*args[:1], 0, *args[2:]) == -2
    assert L.nws_mfcc(*args[:2], 512, *args[3:]) == -2
    assert L.nws_mfcc(*args[:3], 0.0, *args[4:]) == -1
    assert L.nws_mfcc(*args[:4], 1000, *args[5:]) == -1
    assert L.nws_mfcc(*args[:5], 0, *args[6:]) == -1
    assert L.nws_mfcc(*args[:6], 0, *args[7:]) == -1
    assert L.nws_mfcc(*args[:6], 129, *args[7:]) == -1
    assert L.nws_mfcc(*args[:7], 1025, *args[8:]) == -1
    assert L.nws_mfcc(*args[:12], nbytes - 1, None) == -3
    torch.cuda.synchronize()
    assert torch.all(y == 7.0) and torch.all(ws == 0)                  # nothing was launched
    assert L.nws_mfcc(*args) == 0
    torch.cuda.synchronize()
    assert np.array_equal(y[0].cpu().numpy(), _gpu("vibrato_tone"))


def test_loudness_is_bit_identical_around_an_mfcc_call():
    """the two features share the power pass and its DFT operand: a call of one leaves nothing behind for the other"""
    me = _me()
    from nws_amd.data.utils.loudness_extraction import loudness_frames
    g = np.random.default_rng(9)
    a = torch.from_numpy(np.stack([_input("vibrato_tone"), (0.1 * g.standard_normal(6000)).astype(np.float32)])).cuda()
    before = loudness_frames(a, 1024, 128)
    c = me.mfcc_frames(a, *SHIPPED)
    after = loudness_frames(a, 1024, 128)
    c2 = me.mfcc_frames(a, *SHIPPED)
    torch.cuda.synchronize()
    assert before.shape == (2, 47) and torch.equal(before, after) and torch.equal(c, c2)


def test_time_beside_the_loudness_feature():
    """no bar: there is no earlier implementation to compare with.  hipEvents on the launch stream, mean of 3, recorded for
    DESIGN.md 3.11; the two features share the DFT pass, so the ratio says what the mel / dB / DCT passes add"""
    me = _me()
    from nws_amd.data.utils.loudness_extraction import loudness_frames
    g = torch.Generator(device="cuda").manual_seed(3)
    a = 0.3 * torch.randn((64, 64000), device="cuda", generator=g)
    calls = {"mfcc": lambda: me.mfcc_frames(a, *SHIPPED), "loudness": lambda: loudness_frames(a, 1024, 128)}
    ms = {}
    for tag, call in calls.items():
        y = call()                                     # the constant operands' upload is not part of the time
        assert y.shape[0] == 64 and y.shape[-1] == 501
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            call()
        e1.record()
        e1.synchronize()
        ms[tag] = e0.elapsed_time(e1) / 3
        assert np.isfinite(ms[tag]) and ms[tag] > 0
    record("mfcc_time_64x4s", ms_mfcc=ms["mfcc"], ms_loudness=ms["loudness"], ratio=ms["mfcc"] / ms["loudness"],
           x_realtime=a.numel() / 16000 / (ms["mfcc"] * 1e-3))
    print("mfcc", ms["mfcc"], "ms; loudness", ms["loudness"], "ms")
